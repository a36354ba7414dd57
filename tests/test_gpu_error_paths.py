"""Failing calls give back what they took: each error path below runs 200 times on one context, after which the context holds
no more device memory than after its first (warm-up) failure, and still proves bit-exactly.

Every case is an error RETURN that the suite already exercises once somewhere else (a repeated abscissa, a rejected proof, a
prover abandoned half way); none provokes a device fault.  The shapes are the smallest that reach an allocation before the
failure.  After each loop the pool is trimmed and the device's free memory is compared with its value after the warm-up
iteration + trim: it may be lower by at most MAX_DRIFT.  A leak of even the smallest temporaries (KiB-sized blocks times
200, each rounded up by hipMalloc) or of one table per iteration exceeds that; allocator granularity alone does not."""
import random

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from oracle import gkr_ref
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import ProductPoly, SumcheckProof, SumcheckProver, SumcheckVerifier, UnivariatePolynomial, ZkError, gkr

pytestmark = pytest.mark.gpu

FIELD = zk_amd.BN254_FR
LOOPS = 200
MAX_DRIFT = 8 << 20


def free_bytes():
    import torch

    return torch.cuda.mem_get_info(0)[0]


def smoke_proof_bit_exact(ctx):
    """the n = 10, k = 2, D = 2 proof of smoke() against the oracle"""
    n, k, D = 10, 2, 2
    tabs = [orc.fill_random(FIELD, 0x5EED0000 + f, 1 << n) for f in range(k)]
    claimed = orc.sum_elems(FIELD, orc.prod_reduce(FIELD, n, tabs))
    want_rp, want_ch = orc.sumcheck_prove(FIELD, n, tabs, D, claimed, False)
    poly = ProductPoly.new([MLE.new(ctx, n, t) for t in tabs])
    proof, ch = SumcheckProver(D).prove_partial(poly, claimed)
    assert np.array_equal(proof.round_polys, want_rp), "round polynomials differ from the oracle"
    assert np.array_equal(ch, want_ch), "challenges differ from the oracle"


def run_failing(ctx, fail_once):
    """fail_once() runs one failing call and asserts its status"""
    fail_once()                       # warm-up: the pool and the runtime take what they keep
    ctx.synchronize()
    ctx.trim()
    before = free_bytes()
    for _ in range(LOOPS):
        fail_once()
    ctx.synchronize()
    ctx.trim()
    after = free_bytes()
    print(f"free device memory: {before} B after the warm-up, {after} B after {LOOPS} failing calls (drift {before - after} B)")
    assert before - after <= MAX_DRIFT, f"{before - after} bytes of device memory are gone after {LOOPS} failing calls"
    smoke_proof_bit_exact(ctx)        # the context is still usable


def test_interpolate_xy_repeated_abscissa():
    """n = 300 is no power of two: the direct level, one NTT level and the block merges all run before the flag is read"""
    ctx = zk_amd.Context(FIELD, 0)
    n = 300
    xs = zk_amd.fe_from_ints(FIELD, [7 * i + 3 for i in range(n)])
    xs[n - 1] = xs[5]
    xp = UnivariatePolynomial.new(ctx, xs)
    yp = UnivariatePolynomial.new(ctx, orc.fill_random(FIELD, 41, n))

    def fail_once():
        with pytest.raises(ZkError) as e:
            UnivariatePolynomial.interpolate_xy(ctx, xp, yp)
        assert e.value.code == -11   # ZK_ERR_PANIC_INVERSE

    run_failing(ctx, fail_once)
    ctx.close()


def tiny_gkr(ctx):
    """the circuit of smoke() (logs 1, 3, 2) with its honest proof"""
    rng = random.Random(5)
    logs = [1, 3, 2]
    layers = [(logs[i], logs[i + 1], [rng.randrange(2) for _ in range(1 << logs[i])],
               [rng.randrange(1 << logs[i + 1]) for _ in range(1 << logs[i])],
               [rng.randrange(1 << logs[i + 1]) for _ in range(1 << logs[i])]) for i in range(2)]
    inputs = orc.to_ints(FIELD, orc.fill_random(FIELD, 11, 1 << logs[-1]))
    _, want_proof = gkr_ref.gkr_prove(FIELD, layers, inputs, bytes(32))
    circ = gkr.Circuit(ctx)
    for lo, li, op, left, right in layers:
        circ.add_layer(lo, li, op, left, right)
    x = MLE.new(ctx, logs[-1], zk_amd.fe_from_ints(FIELD, inputs))
    out, proof = gkr.gkr_prove(circ, x, bytes(32))
    assert zk_amd.fe_to_ints(FIELD, proof) == want_proof
    assert gkr.gkr_verify(circ, x, out, bytes(32), proof)
    return logs, circ, x, out, proof


# proof layout per layer: [rp #1: log_in * 3 | rp #2: log_in * 3 | W(u) | W(v)]
@pytest.mark.parametrize("what, status", [("sumcheck", -9), ("wv", -27)])
def test_gkr_verify_tampered_proof(what, status):
    """second layer (log_in = 2): an element of its first sumcheck fails the round check (ZK_ERR_VERIFY_SUM) after the first
    layer's tables were enqueued; its W(v) fails the wiring check (ZK_ERR_GKR_REJECT) after every layer's were"""
    from zk_amd._lib import lib
    from zk_amd.api import _p

    ctx = zk_amd.Context(FIELD, 0)
    logs, circ, x, out, proof = tiny_gkr(ctx)
    layer1 = 6 * logs[1] + 2                                   # elements of the first layer's share
    pos = layer1 if what == "sumcheck" else layer1 + 6 * logs[2] + 1
    bad = proof.copy()
    bad[pos] = orc.add(FIELD, bad[pos], zk_amd.fe_from_int(FIELD, 1))
    seed = gkr._seed(bytes(32))

    def fail_once():
        assert lib.zk_gkr_verify(circ._h, x._h, out._h, seed, _p(bad)) == status

    run_failing(ctx, fail_once)
    circ.free()
    ctx.close()


def test_sumcheck_verify_tampered_round():
    ctx = zk_amd.Context(FIELD, 0)
    n, k, D = 10, 2, 2
    tabs = [orc.fill_random(FIELD, 770 + f, 1 << n) for f in range(k)]
    claimed = orc.sum_elems(FIELD, orc.prod_reduce(FIELD, n, tabs))
    poly = ProductPoly.new([MLE.new(ctx, n, t) for t in tabs])
    proof = SumcheckProver(D).prove(poly, claimed)
    assert SumcheckVerifier.verify(poly, proof) is True
    rp = proof.round_polys.copy()
    rp[4, 1] = orc.add(FIELD, rp[4, 1], zk_amd.fe_from_int(FIELD, 1))
    bad = SumcheckProof(proof.sum, rp)

    def fail_once():
        with pytest.raises(ZkError) as e:
            SumcheckVerifier.verify(poly, bad)
        assert e.value.code == -9   # ZK_ERR_VERIFY_SUM

    run_failing(ctx, fail_once)
    ctx.close()


def test_shard_prover_destroyed_mid_proof():
    """rank 0 of a world of 2 (the lanes travel through the host, as with the host transport): one round, then destroyed"""
    from zk_amd.distributed import GpuShardBackend

    ctx = zk_amd.Context(FIELD, 0)
    n, k, D, world = 10, 2, 2, 2
    tabs = [orc.fill_random(FIELD, 880 + f, 1 << n) for f in range(k)]
    claimed = orc.sum_elems(FIELD, orc.prod_reduce(FIELD, n, tabs))
    shards = [np.ascontiguousarray(t[0::world]) for t in tabs]

    def abandon_once():
        poly = ProductPoly.new([MLE.new(ctx, n - 1, s) for s in shards])
        be = GpuShardBackend(poly, D, claimed, world)
        lanes = be.round_begin()
        lanes.copy_(lanes.cpu())      # the exchange point: device -> host -> device
        be.round_finish()
        assert be.local_vars_left() == n - 2
        be.close()

    run_failing(ctx, abandon_once)
    ctx.use_own_stream()
    ctx.close()
