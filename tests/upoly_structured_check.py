"""Univariate products whose transforms hold exact zeros, and all-(p-1) operands (the direct kernel's fe_mul_tt_lazy / fe_add2
accumulation at its worst case), each against a closed form on Python integers.  tests/test_gpu_upoly.py calls run() in its own
process for the default path selection and starts this file in child processes under ZK_UPOLY_DIRECT_MAX (the library reads its ZK_*
switches once per process): 0 sends every product of 2^8 points and more through the fused NTT passes, 2^40 every product to the direct
kernel.

  (1 + x + .. + x^(m-1)) (1 - x) = 1 - x^m      every interior coefficient exactly 0; on the NTT path the truncating inverse stores them
  (1 + x^(N/2)) b, len(b) = N/2                 the first transform is exactly 0 at every odd k (kNttMulStore multiplies by canonical
                                                zeros); the result is b followed by b
  (1 + x^(N/2))^2, (1 - x^(N/4))^2              one handle: kNttSqrStore on a transform with exact zeros
  all-(p-1) times all-(p-1), lengths la, lb     output k is min(k + 1, la, lb, la + lb - 1 - k), since (p - 1)^2 = 1"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import zk_amd  # noqa: E402
from oracle import binding as orc  # noqa: E402
from zk_amd import UnivariatePolynomial as UP  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from upoly_ref import direct_up_to, schoolbook  # noqa: E402

GEOMETRIC_M = (200, 4095, (1 << 16) - 3)
DOUBLING_N = (1 << 8, 1 << 13)


def all_minus_one_shapes():
    x = direct_up_to(4096)   # the longest accumulation the cost model gives the direct kernel at that total
    return [(257, 257), (1000, 3096), (x, 4096 - x)]


def _poly(field, n, terms):
    v = [0] * n
    for k, c in terms.items():
        v[k] = c
    return orc.from_ints(field, v)


def run(field, ctx):
    """every case on `ctx`, under whatever path selection this process has; -> the number of products checked"""
    p = orc.modulus(field)
    E = lambda ints: orc.from_ints(field, ints)  # noqa: E731
    mul = lambda a, b: (UP.new(ctx, a) * UP.new(ctx, b)).coefficients()  # noqa: E731
    done = 0
    one_minus_x = E([1, p - 1])
    for m in GEOMETRIC_M:
        ones = E([1] * m)
        want = _poly(field, m + 1, {0: 1, m: p - 1})
        assert schoolbook(field, [1, p - 1], [1] * m) == orc.to_ints(field, want)
        for got in (mul(ones, one_minus_x), mul(one_minus_x, ones)):
            assert got.shape == (m + 1, 4) and not got[1:m].any(), ("1 - x^m: interior", m)
            assert np.array_equal(got, want), ("1 - x^m", m)
            done += 1
    for N in DOUBLING_N:
        h = N // 2
        b = orc.fill_random(field, 0xD0B1 + N, h)
        a = _poly(field, h + 1, {0: 1, h: 1})
        want = np.concatenate([b, b])
        if N == DOUBLING_N[0]:
            assert schoolbook(field, orc.to_ints(field, a), orc.to_ints(field, b)) == orc.to_ints(field, want)
        for got in (mul(a, b), mul(b, a)):
            assert np.array_equal(got, want), ("(1 + x^(N/2)) b", N)
            done += 1
        for q, sign in ((h, 1), (N // 4, p - 1)):
            s = UP.new(ctx, _poly(field, q + 1, {0: 1, q: sign}))
            got = (s * s).coefficients()
            assert np.array_equal(got, _poly(field, 2 * q + 1, {0: 1, q: 2 * sign % p, 2 * q: 1})), ("square", N, q, sign)
            done += 1
    for la, lb in all_minus_one_shapes():
        a, b = np.tile(orc.from_int(field, p - 1), (la, 1)), np.tile(orc.from_int(field, p - 1), (lb, 1))
        want = E([min(k + 1, la, lb, la + lb - 1 - k) for k in range(la + lb - 1)])
        if la == lb == 257:
            assert schoolbook(field, [p - 1] * la, [p - 1] * lb) == orc.to_ints(field, want)
        for got in (mul(a, b), mul(b, a)):
            assert np.array_equal(got, want), ("all p - 1", la, lb)
            done += 1
    return done


if __name__ == "__main__":
    field = int(sys.argv[1])
    ctx = zk_amd.Context(field, 0)
    try:
        n = run(field, ctx)
    finally:
        ctx.close()
    print(f"upoly structured ok: {n} products (ZK_UPOLY_DIRECT_MAX={os.environ.get('ZK_UPOLY_DIRECT_MAX')})")
