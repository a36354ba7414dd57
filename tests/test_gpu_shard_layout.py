"""Sharding by index mod world on the device (zk_mle_split / zk_mle_interleave / zk_mle_upload_shard): rank g of W holds
{idx : idx mod W == g} with local index idx / W, the layout of the sharded prover and NTT.  Checked against numpy's own strided
reading of the table, as round trips, through the error table of include/zk_amd.h, and by running BASELINE config 3
(n = 24, k = 2, W = 8) and the sharded NTT at 2^24 on shards the device made, on one GPU."""
import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import ProductPoly, ZkError
from zk_amd._lib import c, lib

pytestmark = pytest.mark.gpu

FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]


def _check_split(t, host, world):
    shards = t.split(world)
    assert len(shards) == world
    for g, s in enumerate(shards):
        assert s.n_vars() == t.n_vars() - (world.bit_length() - 1)
        assert np.array_equal(s.evaluation_slice(), host[g::world]), f"world {world}, shard {g}"
    assert MLE.interleave(shards) == t, f"interleave(split(t)) != t at world {world}"


@pytest.mark.parametrize("field", FIELDS)
def test_split_matches_numpy_every_small_size(field):
    ctx = zk_amd.Context(field, 0)
    for n in range(13):
        host = orc.fill_random(field, 900 + n, 1 << n)
        t = MLE.new(ctx, n, host)
        keep = t.clone()
        for w in range(n + 1):
            _check_split(t, host, 1 << w)
        assert t == keep, "split changed its input"
    ctx.close()


@pytest.mark.parametrize("field", FIELDS)
def test_split_matches_numpy_at_2p24(field):
    ctx = zk_amd.Context(field, 0)
    t = MLE.random(ctx, 24, 77 + field)
    host = t.evaluation_slice()
    keep = t.clone()
    for world in (2, 8, 64, 1024):   # direct kernels (2, 8), LDS tiles with the pointers as arguments (64) / in a device table (1024)
        _check_split(t, host, world)
    assert t == keep, "split changed its input"
    ctx.close()


@pytest.mark.parametrize("n", [0, 1, 5, 12, 21])
def test_new_shard_equals_split_of_upload(n):
    field = zk_amd.BLS12_381_FR
    ctx = zk_amd.Context(field, 0)
    host = orc.fill_random(field, 1300 + n, 1 << n)
    full = MLE.new(ctx, n, host)
    for world in sorted({1, 2, 8, 64, 1 << n} if n <= 12 else {1, 2, 8, 64}):
        if world > 1 << n:
            continue
        shards = full.split(world)
        for g in range(world):
            assert MLE.new_shard(ctx, n, host, world, g) == shards[g], f"n {n}, world {world}, rank {g}"
    ctx.close()


def _code(fn, *args):
    with pytest.raises(ZkError) as e:
        fn(*args)
    return e.value.code


def test_shard_layout_error_codes():
    ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
    other = zk_amd.Context(zk_amd.BN254_FR, 0)
    host = orc.fill_random(zk_amd.BN254_FR, 5, 1 << 6)
    t = MLE.new(ctx, 6, host)
    # len != 2^n_vars
    assert _code(MLE.new_shard, ctx, 7, host, 2, 0) == -1
    # world 0, not a power of two, > 2^n_vars, > 2^16; rank >= world
    for world in (0, 3, 12, 128):
        assert _code(MLE.new_shard, ctx, 6, host, world, 0) == -20, world
        assert _code(t.split, world) == -20, world
    big = MLE.random(ctx, 17, 1)
    assert _code(big.split, 1 << 17) == -20
    assert _code(MLE.new_shard, ctx, 6, host, 8, 8) == -20
    # null pointers
    h = c.c_void_p()
    assert lib.zk_mle_upload_shard(ctx._h, 6, None, 64, 2, 0, c.byref(h)) == -20
    assert lib.zk_mle_upload_shard(ctx._h, 6, host.ctypes.data_as(c.POINTER(c.c_uint64)), 64, 2, 0, None) == -20
    assert lib.zk_mle_split(ctx._h, None, 2, (c.c_void_p * 2)()) == -20
    assert lib.zk_mle_split(ctx._h, t._h, 2, None) == -20
    assert lib.zk_mle_interleave(ctx._h, None, 2, c.byref(h)) == -20
    assert lib.zk_mle_interleave(ctx._h, (c.c_void_p * 2)(t._h, None), 2, c.byref(h)) == -20
    assert lib.zk_mle_unshard(ctx._h, None, t._h, c.byref(h)) == -20
    assert _code(MLE.interleave, [t, t, t]) == -20   # three shards: not a power of two
    # shards of different sizes
    assert _code(MLE.interleave, t.split(2)[:1] + t.split(4)[:1]) == -4
    # handles of another context
    assert lib.zk_mle_split(other._h, t._h, 2, (c.c_void_p * 2)()) == -26
    assert _code(MLE.interleave, [t.split(2)[0], MLE.new(other, 5, host[:32])]) == -26
    # a dead communicator: a host transport whose all-gather fails kills it, every later call returns ZK_ERR_COMM
    from zk_amd._lib import HOST_ALLGATHER, HOST_ALLREDUCE

    cbs = (HOST_ALLREDUCE(lambda _u, _b, _n: 0), HOST_ALLGATHER(lambda _u, _s, _n, _r: 1))
    comm = c.c_void_p()
    assert lib.zk_comm_create_host(ctx._h, 1, 0, c.cast(cbs[0], c.c_void_p), c.cast(cbs[1], c.c_void_p), None, None, c.byref(comm)) == 0
    assert lib.zk_mle_unshard(other._h, comm, t._h, c.byref(h)) == -26
    assert lib.zk_mle_unshard(ctx._h, comm, t._h, c.byref(h)) == -28   # the transport fails ...
    assert b"host transport callback returned 1" in lib.zk_last_hip_error()   # (the message is the library's, whichever unit sets it)
    assert lib.zk_mle_unshard(ctx._h, comm, t._h, c.byref(h)) == -28   # ... and the comm is dead
    assert b"communicator is dead" in lib.zk_last_hip_error()
    assert not h.value
    lib.zk_comm_destroy(comm)
    # nothing of the above touched the table
    assert np.array_equal(t.evaluation_slice(), host)
    other.close()
    ctx.close()


# ---- BASELINE config 3 at its own size on one GPU: n = 24, k = 2, D = 2, W = 8, shards made by zk_mle_split ------------------
N3, K3, D3, W3, SEED3 = 24, 2, 2, 8, 0xC0F3


@pytest.fixture(scope="module")
def config3():
    """the oracle's prove_partial of the n = 24 tables (about 8 s on the CPU), computed once"""
    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    polys = [MLE.random(ctx, N3, SEED3, f << N3) for f in range(K3)]   # the _prove_vs_oracle recipe (test_gpu_parity.py)
    tabs = [q.evaluation_slice() for q in polys]
    s = ProductPoly.new(polys).round_sums(1)
    claimed = orc.add(field, s[0], s[1])
    want_rp, want_ch = orc.sumcheck_prove(field, N3, tabs, D3, claimed, False)
    del polys, tabs
    ctx.close()
    return claimed, want_rp, want_ch


@pytest.mark.parametrize("gather_below", [13, 16])
def test_config3_n24_w8_on_device_shards_matches_oracle(config3, gather_below):
    import torch

    from zk_amd.distributed import GpuShardBackend

    claimed, want_rp, want_ch = config3
    ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
    per_factor = []
    for f in range(K3):
        full = MLE.random(ctx, N3, SEED3, f << N3)
        per_factor.append(full.split(W3))   # 8 shards of 2^21
        full.free()
    backends = [GpuShardBackend(ProductPoly.new([per_factor[f][g] for f in range(K3)]), D3, claimed, W3) for g in range(W3)]
    assert backends[0].local_rounds == N3 - 3
    while backends[0].local_vars_left() > gather_below:   # the by-hand all-reduce of tests/test_gpu_shard.py
        lanes = [b.round_begin() for b in backends]
        total = torch.stack(lanes).sum(dim=0)
        for b, lane in zip(backends, lanes):
            lane.copy_(total)
            b.round_finish()
    gathered = torch.cat([b.tail().clone() for b in backends])   # all-gather, rank-major
    for b in backends:
        b.tail_rounds(gathered)
    for g, b in enumerate(backends):
        rp, ch = b.results()
        assert np.array_equal(rp, want_rp), f"rank {g}: round polynomials differ from the oracle"
        assert np.array_equal(ch, want_ch), f"rank {g}: challenges differ from the oracle"
    for b in backends:
        b.close()
    ctx.use_own_stream()
    ctx.close()


def test_sharded_ntt_2p24_w8_on_device_shards():
    """W = 8 GpuNttBackends on shards from split, the all-to-all by hand (tests/test_gpu_shard.py); forward against the sliced
    layout of zk_ntt of the whole vector, inverse put back together by interleave against the input"""
    import torch

    from zk_amd.distributed import GpuNttBackend, sliced_shard_of

    field, n, world = zk_amd.BN254_FR, 24, 8
    ctx = zk_amd.Context(field, 0)
    x = MLE.random(ctx, n, 4242)
    X = zk_amd.ntt(ctx, x, MLE.alloc(ctx, n)).evaluation_slice()

    def exchange(backends):
        sends = [b.send_tensor().view(world, -1) for b in backends]
        for s, b in enumerate(backends):
            b.recv_tensor().view(world, -1).copy_(torch.stack([sends[r][s] for r in range(world)]))

    fw = [GpuNttBackend(s, r, world) for r, s in enumerate(x.split(world))]
    for b in fw:
        b.local_ntt(False)
        b.twiddle(False)
    exchange(fw)
    for r, b in enumerate(fw):
        b.across(False)
        assert np.array_equal(b.result().evaluation_slice(), sliced_shard_of(X, r, world)), f"forward, rank {r}"
    del X
    bw = [GpuNttBackend(b.result(), r, world) for r, b in enumerate(fw)]
    for b in bw:
        b.across(True)
    exchange(bw)
    for b in bw:
        b.twiddle(True)
        b.local_ntt(True)
    assert MLE.interleave([b.result() for b in bw]) == x, "inverse of the forward output, interleaved, is not the input"
    ctx.use_own_stream()
    ctx.close()
