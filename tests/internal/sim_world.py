"""A simulated world of N ranks in one process, on one device.

The bucket protocols of bagua_amd/executor.py take a duck-typed ``comm``.
Here every simulated rank is a Python thread holding its own bucket on the
same device; the collectives are plain torch copies between the ranks'
tensors, separated by a ``threading.Barrier``. The executor functions run
unchanged, so on ``cuda`` they launch the real HIP kernels with
``rank > 0``, real chunk permutations and ``post_scale = 1/n``, which a
single-GPU world of size 1 never does. (Real multi-process worlds are
tests/internal/multi_process.py.)

Every collective snapshots with ``clone()``, waits at the barrier, copies,
and waits again. ``comm.stream`` is None, so all ranks' math and copies go
to the one current stream, where host order is stream order.

This module holds the harness, the input builders, the float64 checks and
the case functions shared by tests/test_sim_world.py (cpu) and
tests/test_gpu_sim_world.py (cuda). It holds no tests.

Bounds follow tests/test_gpu_bucket_kernels.py: k roundings of
``eps32 * mag`` counted from the kernel source, plus half an ulp of the
output type; nothing is tuned to a result.
"""

import collections
import threading
import types

import torch

from tests.test_gpu_bucket_kernels import (
    EPS32,
    _assert_close,
    _bits_equal,
    _half_ulp,
    _name,
)

BARRIER_TIMEOUT = 60.0  # a guard against a broken protocol, not a measurement

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
WORLDS = [2, 3, 8]
CHUNKS = [33, 4096, 4099]


# ---------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------

class _World:
    def __init__(self, n, device):
        self.n = n
        self.device = torch.device(device)
        self.barrier = threading.Barrier(n, timeout=BARRIER_TIMEOUT)
        self.slots = [None] * n
        # FIFO per ordered (sender, receiver) pair
        self.mail = {(s, r): collections.deque()
                     for s in range(n) for r in range(n)}


class SimComm:
    """The communicator surface the bucket protocols use."""

    stream = None

    def __init__(self, world, rank):
        self.world = world
        self.rank_in_comm = rank
        self._recvs = None

    def nranks(self):
        return self.world.n

    def _check(self, t):
        if self.world.device.type == "cuda":
            assert t.is_cuda, "a %s tensor reached a collective of the " \
                "cuda world" % t.device
        assert t.is_contiguous()

    def _exchange(self, t, pick):
        """t's chunk p becomes chunk ``pick(p)`` of rank p's snapshot."""
        w, n = self.world, self.world.n
        self._check(t)
        assert t.numel() % n == 0
        w.slots[self.rank_in_comm] = t.clone().view(n, -1)
        w.barrier.wait()
        tv = t.view(n, -1)
        for p in range(n):
            tv[p].copy_(w.slots[p][pick(p)])
        w.barrier.wait()

    def alltoall_inplace(self, t):
        self._exchange(t, lambda p: self.rank_in_comm)

    def allgather_inplace(self, t):
        self._exchange(t, lambda p: p)

    def group_start(self):
        assert self._recvs is None, "nested group_start"
        self._recvs = []

    def send(self, t, peer):
        assert self._recvs is not None, "send outside a group"
        self._check(t)
        self.world.mail[(self.rank_in_comm, peer)].append(t.clone())

    def recv(self, t, peer):
        assert self._recvs is not None, "recv outside a group"
        self._check(t)
        self._recvs.append((t, peer))

    def group_end(self):
        w = self.world
        recvs, self._recvs = self._recvs, None
        w.barrier.wait()
        for t, peer in recvs:
            t.copy_(w.mail[(peer, self.rank_in_comm)].popleft())
        w.barrier.wait()


class Group:
    """What _HierCtx needs of a process group when hierarchical=False."""

    def __init__(self, comm):
        self._comm = comm

    def get_global_communicator(self):
        return self._comm


def run_world(n, fn, flats):
    """Run ``fn(comm, group, flat)`` once per rank, each in its own thread,
    and return the results by rank. The first exception of any rank breaks
    the barrier for the others and is re-raised here; nothing is retried."""
    assert len(flats) == n
    device = flats[0].device
    assert all(f.device == device for f in flats)
    if device.type == "cuda":
        from bagua_amd.ops import native

        native.require()  # a missing extension must not mean torch fallbacks
    world = _World(n, device)
    results = [None] * n
    errors = []
    lock = threading.Lock()

    def body(rank):
        comm = SimComm(world, rank)
        try:
            results[rank] = fn(comm, Group(comm), flats[rank])
        except BaseException as e:  # noqa: B902 - re-raised in the caller
            with lock:
                errors.append(e)
            world.barrier.abort()

    threads = [threading.Thread(target=body, args=(r,), daemon=True)
               for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        # the ranks that only saw the barrier break are not the cause
        first = [e for e in errors
                 if not isinstance(e, threading.BrokenBarrierError)]
        raise (first or errors)[0]
    if device.type == "cuda":
        torch.cuda.synchronize()
    return results


# ---------------------------------------------------------------------------
# inputs (generated on the CPU from a seed, so that cpu and cuda runs see
# the same values) and checks
# ---------------------------------------------------------------------------

def _seed(tag, n, dtype, chunk):
    return tag * 1000003 + n * 10007 + DTYPES.index(dtype) * 101 + chunk


def _what(proto, n, dtype, chunk, extra=""):
    return ("%s %s n=%d chunk=%d %s" % (proto, _name(dtype), n, chunk,
                                        extra)).strip()


def exact_inputs(n, chunk, dtype, device, hi, seed):
    """Integer buckets whose cross-rank mean is the integer ``base``:
    ranks r and n-1-r hold base + d and base - d with a d of their own,
    the middle rank of an odd world holds base. Everything stays in
    [0, hi]. Every chunk of base has a 0 in its middle and a ``hi`` as its
    last element (in the scalar tail where there is one); d is 0 there, so
    every rank's every chunk has that minimum and maximum too. Returns
    (flats, base[n, chunk] as float64)."""
    g = torch.Generator()
    g.manual_seed(seed)
    base = torch.randint(0, hi + 1, (n, chunk), generator=g)
    base[:, chunk // 2] = 0
    base[:, chunk - 1] = hi
    room = torch.minimum(base, hi - base)
    vals = [None] * n
    for r in range((n + 1) // 2):
        s = n - 1 - r
        if s == r:
            vals[r] = base
            continue
        d = (torch.rand(n, chunk, generator=g) * (room + 1)).floor().long()
        d = torch.minimum(d, room)
        vals[r], vals[s] = base + d, base - d
    assert all(int(v.min()) >= 0 and int(v.max()) <= hi for v in vals)
    assert torch.equal(sum(vals), n * base)
    # the deltas must not vanish, or a misrouted chunk could go unseen
    assert all(bool((vals[r] != base).view(n, -1).any(1).all())
               for r in range(n) if 2 * r != n - 1)
    flats = [v.reshape(-1).to(dtype).to(device) for v in vals]
    return flats, base.double()


def random_inputs(n, chunk, dtype, device, seed):
    """randn * 3 plus a per-rank offset."""
    g = torch.Generator()
    g.manual_seed(seed)
    return [(torch.randn(n * chunk, generator=g) * 3 + (0.5 * r - 1.0))
            .to(dtype).to(device) for r in range(n)]


def _stack64(flats):
    return torch.stack([f.detach().cpu().double() for f in flats])


def assert_within(out, ref64, bound64, what):
    """|out - ref64| <= bound64 elementwise, with the worst ratio printed
    first in the form of _assert_close."""
    out = out.detach().cpu()
    err = (out.double() - ref64).abs()
    ratio = torch.where(bound64 > 0, err / bound64,
                        torch.where(err > 0, torch.full_like(err, 1e30),
                                    torch.zeros_like(err)))
    i = int(ratio.argmax())
    print("BOUND %s n=%d: worst err %.3e at bound %.3e (%.3f of it)"
          % (what, out.numel(), float(err[i]), float(bound64[i]),
             float(ratio[i])))
    assert bool((err <= bound64).all()), (
        "%s: |out-ref64| = %.6e > bound %.6e at index %d"
        % (what, float(err[i]), float(bound64[i]), i))


def assert_all_ranks_equal(outs, what):
    for r in range(1, len(outs)):
        assert _bits_equal(outs[r], outs[0]), (
            "%s: rank %d differs from rank 0" % (what, r))


def assert_bits(out, want64, what):
    """``out`` is bitwise the float64 value ``want64`` cast to its type."""
    want = want64.reshape(-1).to(out.dtype)
    assert bool((want.double() == want64.reshape(-1)).all()), (
        "%s: the expectation is not exact in %s" % (what, out.dtype))
    got = out.detach().cpu()
    if not _bits_equal(got, want):
        bad = (got.double() != want.double()).nonzero().reshape(-1)
        i = int(bad[0]) if bad.numel() else 0
        raise AssertionError(
            "%s: %d of %d elements differ; first at %d: got %r, want %r"
            % (what, bad.numel(), got.numel(), i, float(got[i]),
               float(want[i])))


# ---------------------------------------------------------------------------
# scatter-gather
# ---------------------------------------------------------------------------

def _run_sync(fn_name, flats, average):
    from bagua_amd import executor

    n = len(flats)
    bufs = [f.clone() for f in flats]

    def rank_fn(comm, group, flat):
        getattr(executor, fn_name)(comm, flat, average)

    run_world(n, rank_fn, bufs)
    return bufs


def _exact_hi(n, average):
    """Largest integer of the exact cases: 255 for the mean; for the sum
    255 // n, so that n * base still has 8 significant bits (bf16)."""
    return 255 if average else 255 // n


def case_scattergather_exact(device, n, dtype, chunk, average):
    what = _what("scattergather-exact", n, dtype, chunk,
                 "avg" if average else "sum")
    flats, base = exact_inputs(n, chunk, dtype, device,
                               _exact_hi(n, average),
                               _seed(1, n, dtype, chunk))
    outs = _run_sync("_scattergather_sync", flats, average)
    want = base if average else n * base
    for r in range(n):
        assert_bits(outs[r], want, "%s rank %d" % (what, r))


def case_scattergather_random(device, n, dtype, chunk, average):
    """Rank 0 against the float64 mean or sum; k = n + 1 as for
    reduce_chunk_kernel: n - 1 adds, the reciprocal, the multiply."""
    what = _what("scattergather", n, dtype, chunk,
                 "avg" if average else "sum")
    flats = random_inputs(n, chunk, dtype, device, _seed(2, n, dtype, chunk))
    outs = _run_sync("_scattergather_sync", flats, average)
    assert_all_ranks_equal(outs, what)
    x = _stack64(flats)
    post = 1.0 / n if average else 1.0
    _assert_close(outs[0].cpu(), x.sum(0) * post, x.abs().sum(0) * post,
                  n + 1, what)


# ---------------------------------------------------------------------------
# ByteGrad
# ---------------------------------------------------------------------------

def _quant_error(rng, M):
    """Error of one MinMaxUInt8 round trip before the store to T, for a
    chunk of range ``rng`` (max - min) and largest magnitude ``M``: half a
    level, plus the f32 roundings of x*scale, of the scale itself and of
    the decode, 4 * eps32 * M in the form of _roundtrip_bound of
    tests/test_gpu_bucket_kernels.py. (The clamps of the quantizer fire
    only for M*scale > 2**24.)"""
    return 0.5 * (rng + 1e-7) / 255.0 + 4 * EPS32 * M


def bytegrad_bound(x, dtype, average):
    """(ref64, bound64) of the ByteGrad result, flat, from the float64
    inputs ``x[rank, chunk, i]`` alone. ``hu`` is half an ulp of T (0 for
    f32), evaluated at an upper bound of the magnitude it rounds.

    1. Stage 1, per rank and chunk: the sender's round trip, decoded
       through T:  e1 = a1 + hu(|x| + a1),
       a1 = _quant_error(max - min, max|x|).
    2. The owner of a chunk reduces the n decoded chunks; with post = 1/n
       or 1 the exact reduction is within post * sum_r e1 of
       m = post * sum_r x.
    3. The reduce makes k = n + 1 f32 roundings (as reduce_chunk_kernel)
       of magnitude post * sum_r (|x| + e1), then stores to T:
       e3 = post*sum e1 + k*eps32*mag + hu(|m| + ...).
    4. Stage 2: the reduced chunk lies within w = max_i e3 of m, so its
       range is at most range(m) + 2w and its magnitude max|m| + w:
       total = e3 + a2 + hu(|m| + e3 + a2),
       a2 = _quant_error(range(m) + 2w, max|m| + w).
    """
    n = x.shape[0]
    post = 1.0 / n if average else 1.0

    def hu(v):
        return _half_ulp(v, dtype)

    mn, mx = x.amin(2, keepdim=True), x.amax(2, keepdim=True)
    a1 = _quant_error(mx - mn, x.abs().amax(2, keepdim=True))
    e1 = a1 + hu(x.abs() + a1)
    m = x.sum(0) * post
    e2 = e1.sum(0) * post + (n + 1) * EPS32 * (x.abs() + e1).sum(0) * post
    e3 = e2 + hu(m.abs() + e2)
    w = e3.amax(1, keepdim=True)
    a2 = _quant_error(m.amax(1, keepdim=True) - m.amin(1, keepdim=True)
                      + 2 * w, m.abs().amax(1, keepdim=True) + w)
    total = e3 + a2 + hu(m.abs() + e3 + a2)
    return m.reshape(-1), total.reshape(-1)


def case_bytegrad_exact(device, n, dtype, chunk):
    """Mean only: every chunk on the wire, reduced ones included, spans
    exactly [0, 255], so scale == 1.0f and both quantizations are
    lossless. Sums would leave that range; sum mode runs in the random
    case."""
    what = _what("bytegrad-exact", n, dtype, chunk, "avg")
    flats, base = exact_inputs(n, chunk, dtype, device, 255,
                               _seed(3, n, dtype, chunk))
    outs = _run_sync("_compressed_sync", flats, True)
    for r in range(n):
        assert_bits(outs[r], base, "%s rank %d" % (what, r))


def case_bytegrad_random(device, n, dtype, chunk, average):
    what = _what("bytegrad", n, dtype, chunk, "avg" if average else "sum")
    flats = random_inputs(n, chunk, dtype, device, _seed(4, n, dtype, chunk))
    outs = _run_sync("_compressed_sync", flats, average)
    assert_all_ranks_equal(outs, what)
    ref, bound = bytegrad_bound(_stack64(flats).view(n, n, chunk), dtype,
                                average)
    assert_within(outs[0], ref, bound, what)


# ---------------------------------------------------------------------------
# decentralized shift_one
# ---------------------------------------------------------------------------

class _Holder:
    def __init__(self, t):
        self._t = t

    def tensor(self):
        return self._t


def shift_one_partner(rank, n, step):
    """The half-ring pairing for even n, h = n/2: rank r of the lower half
    meets rank h + (step + r) mod h of the upper half, so rank h + j of
    the upper half meets the r with (step + r) mod h == j."""
    h = n // 2
    if rank < h:
        return h + (step + rank) % h
    return (rank - h - step) % h


def case_shift_one(device, n, dtype, chunk, exact):
    """Steps 0 .. n/2 on one bucket per rank. peer = (x + x_partner) / 2
    is one f32 add (the multiply by 0.5 is exact): k = 1. The exact
    variant uses integers in [-60, 60], whose half sums have at most
    8 significant bits and so are exact in bf16 too."""
    from bagua_amd import executor

    what = _what("shift_one-exact" if exact else "shift_one", n, dtype,
                 chunk)
    numel = n * chunk
    g = torch.Generator()
    g.manual_seed(_seed(5, n, dtype, chunk))
    if exact:
        flats = [torch.randint(-60, 61, (numel,), generator=g).to(dtype)
                 .to(device) for _ in range(n)]
    else:
        flats = [(torch.randn(numel, generator=g) * 3 + (0.5 * r - 1.0))
                 .to(dtype).to(device) for r in range(n)]
    x = _stack64(flats)
    for step in range(n // 2 + 1):
        partner = [shift_one_partner(r, n, step) for r in range(n)]
        assert all(partner[partner[r]] == r and partner[r] != r
                   for r in range(n)), "not an involution: %r" % partner
        bufs = [f.clone() for f in flats]
        peers = [torch.full_like(f, float("nan")) for f in flats]

        def rank_fn(comm, group, flat):
            op = types.SimpleNamespace(
                peer_weight=_Holder(peers[comm.rank_in_comm]),
                hierarchical=False, peer_selection_mode="shift_one",
                step=step)
            executor._exec_decentralized_inner(op, flat, group)

        run_world(n, rank_fn, bufs)
        for r in range(n):
            w = "%s step %d rank %d" % (what, step, r)
            p = partner[r]
            assert _bits_equal(bufs[r], flats[r]), w + ": flat changed"
            assert _bits_equal(peers[r], peers[p]), (
                w + ": differs from its partner %d" % p)
            if exact:
                assert_bits(peers[r], (x[r] + x[p]) * 0.5, w)
        if not exact:
            xp = x[partner]
            _assert_close(torch.cat(peers).cpu(),
                          ((x + xp) * 0.5).reshape(-1),
                          ((x.abs() + xp.abs()) * 0.5).reshape(-1), 1,
                          "%s step %d" % (what, step))


# ---------------------------------------------------------------------------
# low-precision ring
# ---------------------------------------------------------------------------

def low_prec_bound(x, L, R, W, dtype):
    """(ref64, bound64) of the new W of one ring round from that round's
    float64 input state. ``hu`` is half an ulp of T (0 for f32).

    t = x + L/3 + R/3 - 5W/3 is formed by three addmul_inplace, each the
    cast of its factor, a multiply and an add (k = 3) and a store to T:
        et = 9*eps32*mag + 3*hu(mag),  mag = |x| + |L|/3 + |R|/3 + 5|W|/3.
    Its one-chunk round trip, decoded through T, adds
        a + hu(|t| + et + a),  a = _quant_error(range(t) + 2*max et,
                                                 max|t| + max et).
    W_new = d + W is one f32 add of magnitude |d| + |W| and a store to T.
    """
    def hu(v):
        return _half_ulp(v, dtype)

    t = x + L / 3 + R / 3 - 5 * W / 3
    mag = x.abs() + L.abs() / 3 + R.abs() / 3 + 5 * W.abs() / 3
    et = 9 * EPS32 * mag + 3 * hu(mag)
    w = et.max()
    a = _quant_error(t.max() - t.min() + 2 * w, t.abs().max() + w)
    ed = et + a + hu(t.abs() + et + a)
    ref = W + t
    e = ed + EPS32 * (t.abs() + ed + W.abs())
    return ref, e + hu(ref.abs() + e)


def case_low_prec_ring(device, n, dtype, chunk, rounds=3):
    """Three rounds with carried W, L, R. Between rounds every rank moves
    its bucket a little, as an optimizer step would."""
    from bagua_amd import executor

    what = _what("low_prec_ring", n, dtype, chunk)
    numel = n * chunk
    g = torch.Generator()
    g.manual_seed(_seed(6, n, dtype, chunk))

    def rnd(scale):
        return torch.randn(numel, generator=g) * scale

    W = [(rnd(3.0) + (0.5 * r - 1.0)).to(dtype).to(device)
         for r in range(n)]
    L = [W[(r - 1) % n].clone() for r in range(n)]
    R = [W[(r + 1) % n].clone() for r in range(n)]
    flats = [W[r].clone() for r in range(n)]

    def rank_fn(comm, group, flat):
        r = comm.rank_in_comm
        op = types.SimpleNamespace(
            weight=_Holder(W[r]), left_peer_weight=_Holder(L[r]),
            right_peer_weight=_Holder(R[r]), hierarchical=False)
        executor._exec_low_prec_inner(op, flat, group)

    for rd in range(rounds):
        for r in range(n):
            flats[r].add_(rnd(0.1).to(dtype).to(device))
        before = [_stack64(v) for v in (flats, L, R, W)]
        run_world(n, rank_fn, flats)
        for r in range(n):
            w = "%s round %d rank %d" % (what, rd, r)
            assert _bits_equal(L[r], W[(r - 1) % n]), w + ": L != W[left]"
            assert _bits_equal(R[r], W[(r + 1) % n]), w + ": R != W[right]"
            assert _bits_equal(flats[r], W[r]), w + ": flat != W"
        refs = [low_prec_bound(*(b[r] for b in before), dtype)
                for r in range(n)]
        assert_within(torch.cat(W), torch.cat([ref for ref, _ in refs]),
                      torch.cat([bound for _, bound in refs]),
                      "%s round %d" % (what, rd))
