"""UnivariatePolynomial::interpolate / ::interpolate_xy and Add on the device (zk_upoly_interpolate*, zk_upoly_add; univariate_poly.rs
:43-80, :157-184): the reference's KATs, small sizes against the Python restatement (tests/interp_ref.py), xs = omega^i against the
oracle-pinned ifft, exact large-n checks with no host arithmetic, random ys by Schwartz-Zippel, the error table and the C++ mirror."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import UnivariatePolynomial as UP
from zk_amd import ZkError
from zk_amd._lib import c, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interp_ref import RefPanic, lagrange  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
PANIC_INVERSE = -11


@pytest.fixture(params=FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def fctx(request):
    ctx = zk_amd.Context(request.param, 0)
    yield request.param, ctx
    ctx.close()


def _e(field, ints):
    return orc.from_ints(field, [v % orc.modulus(field) for v in ints])


def _i(field, a):
    return orc.to_ints(field, a)


def _rand(field, seed, n):
    return orc.fill_random(field, seed, n) if n else np.zeros((0, 4), dtype=np.uint64)


def test_reference_kats(fctx):
    """test_polynomial_interpolation (:322-350), test_polynomial_addition (:266-293), test_univariate_polynomial_trait_methods (:409-420)"""
    field, ctx = fctx
    p = orc.modulus(field)
    xy = lambda xs, ys: _i(field, UP.interpolate_xy(ctx, _e(field, xs), _e(field, ys)).coefficients())  # noqa: E731
    assert xy([0, 1], [0, 2]) == [0, 2]
    assert xy([0, 1, 2], [5, 7, 13]) == [5, 0, 2]
    # the reference's expected vector [12, 25, 18, 24, 12, 8] is read mod 17 (its Fq); the exact integer polynomial its comment
    # states, 8x^5 + 12x^4 + 7x^3 + x^2 + 8x + 12, is what holds in every field
    assert xy([0, 1, 3, 4, 5, 8], [12, 48, 3150, 11772, 33452, 315020]) == [12, 8, 1, 7, 12, 8]
    assert xy([5, 7, 9, 1], [565, 1631, 3537, -7]) == [0, p - 12, 0, 5]
    P = lambda v: UP.new(ctx, _e(field, v))  # noqa: E731
    zero = P([])
    z = zero + zero
    assert z.len() == 0 and z == zero
    assert _i(field, (zero + P([0, 2])).coefficients()) == [0, 2]
    assert _i(field, (P([0, 2]) + zero).coefficients()) == [0, 2]
    a, b = P([4, 3, 2]), P([3, 4, 0, 4])
    assert a + b == b + a
    assert _i(field, (a + b).coefficients()) == [7, 7, 2, 4]
    q = UP.interpolate_xy(ctx, _e(field, [5, 7, 9, 1]), _e(field, [565, 1631, 3537, -7]))
    assert q + zero == q
    assert orc.to_int(field, q.evaluate(orc.from_u64(field, 5))) == 565
    assert _i(field, (P([1, 2, 0]) + P([p - 1])).coefficients()) == [0, 2, 0]   # nothing trimmed


def test_interpolate_small_sizes_against_restatement(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    sizes = list(range(0, 41)) + [127, 128, 129, 255, 256, 257, 383, 384, 385, 513]
    for n in sizes:
        ys = _rand(field, 100 + n, n)
        got = UP.interpolate(ctx, ys)
        assert got.len() == n
        assert _i(field, got.coefficients()) == lagrange(list(range(n)), _i(field, ys), p), n
    assert UP.interpolate(ctx, np.zeros((0, 4), dtype=np.uint64)).len() == 0
    # trailing zeros are kept: a constant interpolated over 5 points
    assert _i(field, UP.interpolate(ctx, _e(field, [7] * 5)).coefficients()) == [7, 0, 0, 0, 0]


def test_interpolate_xy_shapes_and_duplicates(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(field)
    for nx, ny in [(1, 1), (5, 3), (3, 5), (0, 4), (4, 0), (0, 0), (40, 40), (70, 33), (33, 70), (300, 300), (300, 129)]:
        xs = [rng.randrange(p) for _ in range(nx)]
        ys = [rng.randrange(p) for _ in range(ny)]
        got = UP.interpolate_xy(ctx, _e(field, xs), _e(field, ys))
        want = lagrange(xs, ys, p)
        assert got.len() == len(want) == (nx if min(nx, ny) else 0)
        assert _i(field, got.coefficients()) == want, (nx, ny)
        if nx and ny:
            assert _i(field, zk_amd.upoly_interpolate_host(ctx, _e(field, ys), _e(field, xs))) == want
    # duplicates: an error exactly when one of the two indices is < m
    for xs, ny, bad in [([1, 2, 1, 4], 4, True), ([1, 2, 3, 4, 3], 3, True), ([1, 2, 3, 5, 5], 3, False), ([9, 9], 1, True),
                        ([1, 2, 3, 4, 4, 4], 4, True), ([1, 2, 3, 7, 7, 7], 3, False)]:
        ys = [rng.randrange(p) for _ in range(ny)]
        try:
            want = lagrange(xs, ys, p)
        except RefPanic:
            want = None
        assert (want is None) == bad
        if bad:
            with pytest.raises(ZkError) as e:
                UP.interpolate_xy(ctx, _e(field, xs), _e(field, ys))
            assert e.value.code == PANIC_INVERSE
        else:
            assert _i(field, UP.interpolate_xy(ctx, _e(field, xs), _e(field, ys)).coefficients()) == want


# one n in each regime of upoly_interp_tree: direct LDS levels only (largest block below 2^8), the first batched-NTT level with
# 2^8 - 1 and 2^8 + 1 around it, and several batched levels with block merges
LOW_DEGREE_SIZES = [100, 255, 256, 257, 2100]


def _low_degree_polys(field):
    """degrees 0, 1, 3 with every coefficient 1, every coefficient p - 1, and random ones; one mix of the three; and zero"""
    p = orc.modulus(field)
    rng = random.Random(0x1A7E + field)
    qs = [[0]]
    for d in (0, 1, 3):
        qs += [[1] * (d + 1), [p - 1] * (d + 1), [rng.randrange(1, p) for _ in range(d + 1)]]
    return qs + [[p - 1, 1, rng.randrange(1, p), p - 1]]


def _poly_at(p, q, x):
    acc = 0
    for co in reversed(q):
        acc = (acc * x + co) % p
    return acc


@pytest.mark.parametrize("n", LOW_DEGREE_SIZES)
def test_interpolating_a_low_degree_polynomial_pads_with_exact_zeros(fctx, n):
    """ys[j] = q(j), deg q <= 3: interpolate returns q's coefficients followed by n - deg q - 1 exact zeros, so every tree level
    (direct, kNttBatchPad / kNttBatchCombine / kNttBatchShift, the merges' products) works on operands that cancel to zero.  ys all
    zero and ys all p - 1 are the first cases.  interpolate_xy at a seeded permutation of distinct xs holding 0, 1 and p - 1 gives
    the same padded result."""
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(n * 3 + field)
    xs = {0, 1, p - 1}
    while len(xs) < n:
        xs.add(rng.randrange(p))
    xs = sorted(xs)
    rng.shuffle(xs)
    xs_dev = UP.new(ctx, _e(field, xs))
    qs = _low_degree_polys(field)
    assert len(qs) == 11
    for q in qs:
        want = _e(field, q + [0] * (n - len(q)))
        got = UP.interpolate(ctx, _e(field, [_poly_at(p, q, j) for j in range(n)])).coefficients()
        assert np.array_equal(got, want), ("interpolate", n, q)
        got = UP.interpolate_xy(ctx, xs_dev, UP.new(ctx, _e(field, [_poly_at(p, q, x) for x in xs]))).coefficients()
        assert np.array_equal(got, want), ("interpolate_xy", n, q)
    ys = _i(field, UP.interpolate(ctx, _e(field, [p - 1] * n)).coefficients())
    assert ys == [p - 1] + [0] * (n - 1)


def test_stale_pool_data_under_the_inputs():
    """the inputs' and the temporaries' pool blocks hold stale nonzero words (freed random tables of the same size classes)"""
    field = zk_amd.BLS12_377_FR
    p = orc.modulus(field)
    ctx = zk_amd.Context(field, 0)
    for n in ((1 << 9) - 3, (1 << 10) - 1, 600):
        for n_vars in (9, 10, 11):
            for s in range(4):
                MLE.random(ctx, n_vars, 77 + s + n_vars).free()
        ys = _rand(field, 5 + n, n)
        got = _i(field, UP.interpolate(ctx, ys).coefficients())
        assert got == lagrange(list(range(n)), _i(field, ys), p), n
    ctx.close()


@pytest.mark.parametrize("log_n", [10, 14, 16])
def test_roots_of_unity_match_ifft(log_n):
    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    n = 1 << log_n
    e1 = np.zeros((n, 4), dtype=np.uint64)
    e1[1] = orc.from_u64(field, 1)
    xs = zk_amd.fft(ctx, e1)   # fft of e_1: omega^i
    ys = _rand(field, 3000 + log_n, n)
    got = UP.interpolate_xy(ctx, xs, ys).coefficients()
    assert np.array_equal(got, zk_amd.ifft(ctx, ys))
    ctx.close()


def _raw_quadratic(n, a):
    i = np.arange(n, dtype=np.uint64)
    raw = np.zeros((n, 4), dtype=np.uint64)
    raw[:, 0] = np.uint64(a[0]) + np.uint64(a[1]) * i + np.uint64(a[2]) * i * i
    return raw


@pytest.mark.parametrize("field,n", [(zk_amd.BN254_FR, 1 << 24)] + [(f, (1 << 20) + 3) for f in FIELDS])
def test_large_interpolate_of_a_quadratic_is_exact(field, n):
    """raw limbs [c(i), 0, 0, 0] are R^-1 c(i), still a quadratic in i: the result's raw limbs are [a0], [a1], [a2] and n - 3 zeros"""
    ctx = zk_amd.Context(field, 0)
    a = (11111, 2345, 13)
    got = UP.interpolate(ctx, _raw_quadratic(n, a)).coefficients()
    assert got.shape == (n, 4)
    want_head = np.zeros((3, 4), dtype=np.uint64)
    want_head[:, 0] = a
    assert np.array_equal(got[:3], want_head)
    assert not got[3:].any()
    ctx.close()


def _barycentric(p, ys, z):
    """r(z) = M(z) sum_i w_i / (z - i), xs = 0 .. n-1, w_i = y_i (-1)^(n-1-i) / (i! (n-1-i)!)"""
    n = len(ys)
    fact = [1] * n
    for k in range(1, n):
        fact[k] = fact[k - 1] * k % p
    inv_last = pow(fact[n - 1], p - 2, p)
    inv_fact = [0] * n
    inv_fact[n - 1] = inv_last
    for k in range(n - 1, 0, -1):
        inv_fact[k - 1] = inv_fact[k] * k % p
    diffs = [(z - i) % p for i in range(n)]
    M = 1
    for d in diffs:
        M = M * d % p
    pre = [1] * (n + 1)   # batch inversion of the differences
    for k in range(n):
        pre[k + 1] = pre[k] * diffs[k] % p
    inv = pow(pre[n], p - 2, p)
    acc = 0
    for k in range(n - 1, -1, -1):
        inv_d = inv * pre[k] % p
        inv = inv * diffs[k] % p
        w = ys[k] * inv_fact[k] * inv_fact[n - 1 - k] % p
        acc = (acc - w * inv_d) if (n - 1 - k) & 1 else (acc + w * inv_d)
    return M * acc % p


@pytest.mark.parametrize("field,n", [(f, (1 << 16) + d) for f in FIELDS for d in (-1, 1)] + [(zk_amd.BN254_FR, 1 << 20)])
def test_random_ys_schwartz_zippel(field, n):
    ctx = zk_amd.Context(field, 0)
    p = orc.modulus(field)
    ys = _rand(field, 70 + n, n)
    r = UP.interpolate(ctx, ys)
    assert r.len() == n
    rng = random.Random(n)
    for i in rng.sample(range(n), 64):
        assert np.array_equal(r.evaluate(orc.from_u64(field, i)), ys[i])
    z = rng.randrange(n, p)
    assert orc.to_int(field, r.evaluate(_e(field, [z])[0])) == _barycentric(p, _i(field, ys), z)
    ctx.close()


def test_error_table():
    field = zk_amd.BN254_FR
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    a = UP.new(ctx, _rand(field, 1, 8))
    b_other = UP.new(other, _rand(field, 2, 8))
    out = np.zeros((16, 4), dtype=np.uint64)
    h = c.c_void_p()
    u64p = c.POINTER(c.c_uint64)
    p = lambda v: v.ctypes.data_as(u64p)  # noqa: E731
    BAD, MISMATCH, UNSUP = -20, -26, -25
    assert lib.zk_upoly_add(ctx._h, a._h, None, c.byref(h)) == BAD
    assert lib.zk_upoly_add(ctx._h, a._h, a._h, None) == BAD
    assert lib.zk_upoly_add(None, a._h, a._h, c.byref(h)) == BAD
    assert lib.zk_upoly_interpolate(ctx._h, None, c.byref(h)) == BAD
    assert lib.zk_upoly_interpolate(ctx._h, a._h, None) == BAD
    assert lib.zk_upoly_interpolate_xy(ctx._h, a._h, None, c.byref(h)) == BAD
    assert lib.zk_upoly_interpolate_xy(ctx._h, None, a._h, c.byref(h)) == BAD
    assert lib.zk_upoly_interpolate_host(ctx._h, None, 3, p(out)) == BAD
    assert lib.zk_upoly_interpolate_host(ctx._h, p(out), 3, None) == BAD
    assert lib.zk_upoly_interpolate_xy_host(ctx._h, p(out), 3, p(out), 3, None) == BAD
    assert lib.zk_upoly_interpolate_xy_host(ctx._h, None, 3, p(out), 3, p(out)) == BAD
    assert lib.zk_upoly_add(ctx._h, a._h, b_other._h, c.byref(h)) == MISMATCH
    assert lib.zk_upoly_add(other._h, a._h, a._h, c.byref(h)) == MISMATCH
    assert lib.zk_upoly_interpolate(other._h, a._h, c.byref(h)) == MISMATCH
    assert lib.zk_upoly_interpolate_xy(ctx._h, a._h, b_other._h, c.byref(h)) == MISMATCH
    # the length rule, checked before the (short) inputs are read: 2^ceil(log2 n) past 2^two_adicity / 2^32
    s = zk_amd.two_adicity(field)
    assert lib.zk_upoly_interpolate_host(ctx._h, p(out), (1 << s) + 1, p(out)) == UNSUP
    assert lib.zk_upoly_interpolate_xy_host(ctx._h, p(out), (1 << s) + 1, p(out), 1, p(out)) == UNSUP
    assert lib.zk_upoly_interpolate_host(ctx._h, p(out), (1 << 32) + 1, p(out)) == UNSUP
    # empty results: nothing written, out may be NULL
    assert lib.zk_upoly_interpolate_host(ctx._h, p(out), 0, None) == 0
    assert lib.zk_upoly_interpolate_xy_host(ctx._h, p(out), 0, p(out), 3, None) == 0
    # a repeated x: the error, and no handle
    xs = UP.new(ctx, _e(field, [3, 4, 3]))
    ys = UP.new(ctx, _e(field, [1, 2, 3]))
    h = c.c_void_p()
    assert lib.zk_upoly_interpolate_xy(ctx._h, xs._h, ys._h, c.byref(h)) == PANIC_INVERSE
    assert not h.value
    assert lib.zk_upoly_interpolate_xy_host(ctx._h, p(_e(field, [3, 4, 3])), 3, p(_e(field, [1, 2, 3])), 3, p(out)) == PANIC_INVERSE
    with pytest.raises(ZkError) as e:
        a + b_other
    assert e.value.code == MISMATCH
    for q in (a, b_other, xs, ys):
        q.free()
    ctx.close()
    other.close()


def test_cpp_host_mirror_kats_and_2p20_interpolate(tmp_path):
    """tests/cpp/test_upoly_interp.cpp over zk.hpp: the KATs, Add and one 2^20 interpolate of a raw-limb quadratic"""
    exe = str(tmp_path / "test_upoly_interp")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_upoly_interp.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: upoly interpolation host tests passed" in r.stdout
