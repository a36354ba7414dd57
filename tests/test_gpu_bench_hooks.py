"""Each of the sixteen zk_bench_* measurement hooks once, reps = 2, at the smallest shapes at which its paths exist: the status, the
returned times (finite, positive, the documented number of them), the phase arrays of the three phase-timed hooks (zeros on a direct
path, a split on the tree / Newton path, no phase longer than the call), the sample count of fold_samples for a group that does not
divide reps, and a context that is still usable after a hook has refused its arguments."""
import math

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import DeviceCoeffMultilinear as DC
from zk_amd import MerkleTree
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import UnivariatePolynomial as UP
from zk_amd import ZkError
from zk_amd._lib import c, lib

pytestmark = pytest.mark.gpu

FIELD = zk_amd.BN254_FR
REPS = 2
BAD = -20


@pytest.fixture(scope="module")
def ctx():
    ctx = zk_amd.Context(FIELD, 0)
    yield ctx
    ctx.close()


def _time(v):
    assert math.isfinite(v) and v > 0, v
    return v


def _phases(ms, n, split):
    """ms[0] the call, ms[1..n) its phases: all zero where the path has no split, else none negative or longer than the call"""
    vals = [float(v) for v in ms]
    assert len(vals) == n and all(math.isfinite(v) for v in vals), vals
    _time(vals[0])
    if not split:
        assert all(v == 0.0 for v in vals[1:]), vals
    else:
        assert all(0.0 <= v <= vals[0] for v in vals[1:]) and any(v > 0 for v in vals[1:]), vals


def test_fold_and_samples(ctx):
    t, out = MLE.random(ctx, 10, 1), MLE.alloc(ctx, 9)
    r = orc.fill_random(FIELD, 2, 1)
    _time(t.bench_fold(r, out, REPS))
    assert out == t.fold_into(r, MLE.alloc(ctx, 9))   # the hook's launches are the fold itself
    for reps, group in ((5, 2), (2, 1), (3, 4)):
        ms = t.bench_fold_samples(r, out, reps, group=group)
        assert len(ms) == -(-reps // group)
        for v in ms:
            _time(float(v))
    # an argument error leaves the context usable: the same hook runs right after it
    bad_out, ms1 = MLE.alloc(ctx, 10), c.c_double(-1.0)
    rp = np.ascontiguousarray(r, dtype=np.uint64).ctypes.data_as(c.POINTER(c.c_uint64))
    assert lib.zk_bench_fold(ctx._h, t._h, rp, bad_out._h, REPS, c.byref(ms1)) == BAD and ms1.value == -1.0
    assert lib.zk_bench_fold_samples(ctx._h, t._h, rp, out._h, REPS, 0, c.byref(ms1)) == BAD and ms1.value == -1.0
    _time(t.bench_fold(r, out, REPS))
    assert len(t.bench_fold_samples(r, out, REPS)) == REPS


def test_wall_clock_hooks(ctx):
    n = 10
    tabs = [MLE.random(ctx, n, 3 + f) for f in range(2)]
    host = [t.evaluation_slice() for t in tabs]
    claimed = orc.sum_elems(FIELD, orc.prod_reduce(FIELD, n, host))
    each = zk_amd.bench_prove_partial(zk_amd.ProductPoly.new(tabs), 2, claimed, reps=REPS)
    assert len(each) == REPS
    for v in each:
        _time(v)
    pt = orc.fill_random(FIELD, 5, n)
    each = zk_amd.bench_evaluate(tabs[0], pt, reps=REPS)
    assert len(each) == REPS
    for v in each:
        _time(v)
    _time(zk_amd.bench_evaluate_device(tabs[0], pt, reps=REPS))
    with pytest.raises(ZkError):   # the arity is checked before anything runs; the context takes the next call
        zk_amd.bench_evaluate_device(tabs[0], pt[:-1], reps=REPS)
    _time(zk_amd.bench_evaluate_device(tabs[0], pt, reps=REPS))


def test_modmul_and_copy(ctx):
    for variant in (0, 1):
        _time(ctx.bench_modmul(iters=16, variant=variant))
    _time(ctx.bench_copy(1 << 16, reps=REPS))
    with pytest.raises(ZkError):
        ctx.bench_copy(8, reps=REPS)
    _time(ctx.bench_copy((1 << 16) + 16, reps=REPS))


def test_ntt(ctx):
    a, b = MLE.random(ctx, 10, 7), MLE.alloc(ctx, 10)
    for inverse in (False, True):
        _time(zk_amd.bench_ntt(ctx, a, b, inverse=inverse, reps=REPS))


def test_upoly_interp_phases(ctx):
    ms = (c.c_double * 5)()
    for n in (100, 1024):   # direct tree levels only with block merges; NTT levels
        ys = UP.new(ctx, orc.fill_random(FIELD, 11, n))
        assert lib.zk_bench_upoly_interp(ctx._h, None, ys._h, REPS, ms) == 0
        _phases(ms, 5, True)
    n = 600   # interpolate_xy: NTT levels and merges
    xs, ys = UP.new(ctx, orc.from_ints(FIELD, list(range(3, 3 + n)))), UP.new(ctx, orc.fill_random(FIELD, 12, n))
    assert lib.zk_bench_upoly_interp(ctx._h, xs._h, ys._h, REPS, ms) == 0
    _phases(ms, 5, True)
    assert lib.zk_bench_upoly_interp(ctx._h, xs._h, ys._h, 0, ms) == BAD
    assert lib.zk_bench_upoly_interp(ctx._h, xs._h, ys._h, 1, ms) == 0


def test_upoly_evaluate_many_phases(ctx):
    ms = (c.c_double * 6)()
    p, xs = UP.new(ctx, orc.fill_random(FIELD, 13, 300)), UP.new(ctx, orc.fill_random(FIELD, 14, 500))
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, p._h, xs._h, 1, REPS, ms) == 0   # forced direct
    _phases(ms, 6, False)
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, p._h, xs._h, 2, REPS, ms) == 0   # forced tree
    _phases(ms, 6, True)
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, p._h, xs._h, 0, REPS, ms) == 0   # the switch
    _time(ms[0])
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, p._h, xs._h, 3, REPS, ms) == BAD
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, p._h, xs._h, 2, 1, ms) == 0


def test_upoly_divrem_phases(ctx):
    ms = (c.c_double * 4)()
    a, b = UP.new(ctx, orc.fill_random(FIELD, 15, 700)), UP.new(ctx, orc.fill_random(FIELD, 16, 130))
    two = UP.new(ctx, orc.fill_random(FIELD, 17, 2))
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 1, REPS, ms) == 0   # direct
    _phases(ms, 4, False)
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, two._h, 2, REPS, ms) == 0   # linear divisor
    _phases(ms, 4, False)
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 3, REPS, ms) == 0   # Newton
    _phases(ms, 4, True)
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 0, REPS, ms) == 0   # the switches
    _time(ms[0])
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 2, REPS, ms) == BAD   # the linear path wants lb = 2
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 3, 1, ms) == 0


def test_cmle_hooks(ctx):
    n = 10
    t = MLE.random(ctx, n, 21)
    d = DC.interpolate(ctx, t)
    pt = orc.fill_random(FIELD, 22, n)
    for op in range(3):
        _time(d.bench(op, table=t, point=pt, reps=REPS))
    other = DC.upload(ctx, n, orc.fill_random(FIELD, 23, 1 << n))
    small = DC.upload(ctx, 5, orc.fill_random(FIELD, 24, 1 << 5))
    selector = [i == 1 for i in range(n)]
    _time(d.bench_algebra(0, assignments=[(selector, orc.from_ints(FIELD, [5])[0])], reps=REPS))
    _time(d.bench_algebra(1, other=other, reps=REPS))
    _time(d.bench_algebra(2, scalar=orc.from_ints(FIELD, [9])[0], reps=REPS))
    _time(small.bench_algebra(3, other=small, reps=REPS))
    with pytest.raises(ZkError):   # the warm call finds the error; the next call runs
        d.bench_algebra(4, reps=REPS)
    with pytest.raises(ZkError):
        d.bench(3, table=t, point=pt, reps=REPS)
    _time(d.bench_algebra(1, other=other, reps=REPS))
    _time(d.bench(1, reps=REPS))


def test_batch_inverse_merkle_fri(ctx):
    t, o = MLE.random(ctx, 10, 31), MLE.alloc(ctx, 10)
    for path in range(4):   # the switch, one launch, three launches, prefix product
        _time(t.bench_batch_inverse(o, path=path, reps=REPS))
    with pytest.raises(ZkError):
        t.bench_batch_inverse(o, path=4, reps=REPS)
    _time(t.bench_batch_inverse(o, path=0, reps=REPS))
    assert o == t.batch_inverse()
    cols = [t, MLE.random(ctx, 10, 32)]
    for path in range(3):   # the switch, fused stages, one launch per level
        _time(MerkleTree.bench(cols, path=path, reps=REPS))
    with pytest.raises(ZkError):
        MerkleTree.bench(cols, path=3, reps=REPS)
    _time(MerkleTree.bench(cols, path=0, reps=REPS))
    for arity, out in ((1, MLE.alloc(ctx, 9)), (3, MLE.alloc(ctx, 7))):
        for path in range(3):   # the switch, the fused kernel, binary launches
            _time(zk_amd.bench_fri_fold(t, arity, out, path=path, reps=REPS))
    with pytest.raises(ZkError):
        zk_amd.bench_fri_fold(t, 1, MLE.alloc(ctx, 7), reps=REPS)
    _time(zk_amd.bench_fri_fold(t, 1, MLE.alloc(ctx, 9), reps=REPS))
