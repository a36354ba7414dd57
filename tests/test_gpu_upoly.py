"""UnivariatePolynomial on the device (zk_upoly_*, polynomial/src/univariate_poly.rs): the reference's own KATs, products against
a Python big-int schoolbook product and against an independent CPU composition of oracle primitives (ntt_fast, prod_reduce,
inverse ntt_fast, truncate), both product paths forced in child processes, evaluate against Horner, and the error table."""
import hashlib
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import UnivariatePolynomial as UP
from zk_amd import ZkError
from zk_amd._lib import c, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from upoly_ref import direct_up_to, schoolbook  # noqa: E402
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]


def _ints(field, a):
    return orc.to_ints(field, a)


def _elems(field, ints):
    return orc.from_ints(field, ints)


def schoolbook_at(field, a, b, k):
    p = orc.modulus(field)
    return sum(a[i] * b[k - i] for i in range(max(0, k - len(b) + 1), min(k, len(a) - 1) + 1)) % p


def horner(field, coeffs, x):
    p = orc.modulus(field)
    acc = 0
    for co in reversed(coeffs):
        acc = (acc * x + co) % p
    return acc


def _rand(field, seed, n):
    return orc.fill_random(field, seed, n) if n else np.zeros((0, 4), dtype=np.uint64)


def _mul(ctx, a, b):
    return (UP.new(ctx, a) * UP.new(ctx, b)).coefficients()


@pytest.fixture(params=FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def fctx(request):
    ctx = zk_amd.Context(request.param, 0)
    yield request.param, ctx
    ctx.close()


def test_reference_kats(fctx):
    """univariate_poly.rs:257-319 restated with small integers (the mod-17 results become the exact integer products)"""
    field, ctx = fctx
    P = lambda v: UP.new(ctx, _elems(field, v))  # noqa: E731
    p, q = P([4, 3, 2]), P([3, 4, 0, 4])
    assert _ints(field, (p * q).coefficients()) == [12, 25, 18, 24, 12, 8]
    assert p * q == q * p
    for z in (P([]) * P([0, 2]), P([0, 2]) * P([]), P([]) * P([])):
        assert z.len() == 0 and z.coefficients().shape == (0, 4)
    assert _ints(field, (P([0]) * P([1, 2, 3])).coefficients()) == [0, 0, 0]   # nothing trimmed
    assert _ints(field, (P([1, 0, 0]) * P([1, 0])).coefficients()) == [1, 0, 0, 0]
    assert orc.to_int(field, P([0, 2]).evaluate(orc.from_u64(field, 4))) == 8    # test_evaluation
    assert orc.to_int(field, P([]).evaluate(orc.from_u64(field, 4))) == 0


def _grid():
    g = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2), (2, 7)]
    for total in (1000, 4096):   # around the crossover, both paths and both operand orders
        x = direct_up_to(total)
        for m in range(x - 2, x + 3):
            g += [(m, total - m), (total - m, m)]
    for k in (8, 12, 16):   # la + lb - 1 = 2^k and 2^k + 1
        lb = 40 if k == 16 else (1 << (k - 1)) - 3 if k == 8 else 300
        for lc in (1 << k, (1 << k) + 1):
            g.append((lc + 1 - lb, lb))
    g += [(128, 129), (129, 128)]   # balanced, N = 2^8
    return g


def test_products_against_schoolbook(fctx):
    field, ctx = fctx
    for n, (la, lb) in enumerate(_grid()):
        a, b = _rand(field, 10 * n + 1, la), _rand(field, 10 * n + 2, lb)
        got = _mul(ctx, a, b)
        assert got.shape == (la + lb - 1 if la and lb else 0, 4), (la, lb)
        assert _ints(field, got) == schoolbook(field, _ints(field, a), _ints(field, b)), (la, lb)


def test_lopsided_squaring_and_trailing_zeros(fctx):
    field, ctx = fctx
    # 1 x 2^16: every output
    a, b = _rand(field, 71, 1), _rand(field, 72, 1 << 16)
    assert _ints(field, _mul(ctx, a, b)) == schoolbook(field, _ints(field, a), _ints(field, b))
    # 3 x 2^20 (direct) and 60 x 2^20 (NTT path): sampled outputs
    rng = random.Random(field)
    for ls in (3, 60):
        a, b = _rand(field, 73 + ls, ls), _rand(field, 74 + ls, 1 << 20)
        got, ai, bi = _ints(field, _mul(ctx, a, b)), _ints(field, a), _ints(field, b)
        assert len(got) == ls + (1 << 20) - 1
        for k in [0, 1, 2, len(got) - 1, len(got) - 2] + [rng.randrange(len(got)) for _ in range(200)]:
            assert got[k] == schoolbook_at(field, ai, bi, k), (ls, k)
    # squaring through the same handle, both paths
    for la in (20, 300, 1000):
        a = _rand(field, 80 + la, la)
        h = UP.new(ctx, a)
        sq = h * h
        assert _ints(field, sq.coefficients()) == schoolbook(field, _ints(field, a), _ints(field, a)), la
        assert np.array_equal(h.coefficients(), a)
    # trailing zeros on either side keep the length
    for la, lb, za, zb in [(10, 5, 3, 0), (300, 200, 0, 50), (1000, 64, 500, 63)]:
        a, b = _rand(field, 90 + la, la), _rand(field, 91 + lb, lb)
        a[la - za:], b[lb - zb:] = 0, 0
        got = _mul(ctx, a, b)
        assert got.shape[0] == la + lb - 1
        assert _ints(field, got) == schoolbook(field, _ints(field, a), _ints(field, b))
    assert _ints(field, _mul(ctx, _elems(field, [0] * 100), _rand(field, 95, 400))) == [0] * 499


def _oracle_product(field, a, b):
    """independent CPU composition of oracle primitives: ntt_fast on padded inputs, prod_reduce, inverse ntt_fast, truncate"""
    lc = a.shape[0] + b.shape[0] - 1
    n = 1 << (lc - 1).bit_length()
    pa, pb = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    pa[:a.shape[0]], pb[:b.shape[0]] = a, b
    with ThreadPoolExecutor(2) as ex:   # the oracle call releases the GIL
        fa, fb = ex.map(lambda v: orc.ntt_fast(field, v), [pa, pb])
    prod = orc.prod_reduce(field, n.bit_length() - 1, [fa, fb])
    return orc.ntt_fast(field, prod, inverse=True)[:lc]


@pytest.mark.parametrize("field,log_n", [(f, 20) for f in FIELDS] + [(zk_amd.BN254_FR, 24), (zk_amd.BLS12_381_FR, 25)])
def test_large_products_against_oracle_composition(field, log_n):
    ctx = zk_amd.Context(field, 0)
    la = lb = 1 << (log_n - 1)
    if log_n == 20:
        lb -= 1000   # uneven operands, still N = 2^20
    a, b = _rand(field, 500 + log_n, la), _rand(field, 600 + log_n, lb)
    A, B = UP.new(ctx, a), UP.new(ctx, b)
    C = A * B
    got = C.coefficients()
    assert got.shape == (la + lb - 1, 4)
    assert np.array_equal(got, _oracle_product(field, a, b))
    # C(z) == A(z) * B(z), and the inputs are unchanged
    z = orc.fill_random(field, 7 + log_n, 1)[0]
    assert np.array_equal(C.evaluate(z), orc.mul(field, A.evaluate(z), B.evaluate(z)))
    assert np.array_equal(A.coefficients(), a) and np.array_equal(B.coefficients(), b)
    ctx.close()


def test_pad_on_load_reads_nothing_past_len():
    """the operand's pool block holds stale nonzero words past its end: a freed 2^12-element random table of the same size class"""
    field = zk_amd.BLS12_377_FR
    ctx = zk_amd.Context(field, 0)
    for la, lb in [((1 << 12) - 7, 300), (2000, (1 << 11) - 1)]:
        for n_vars in (11, 12):
            MLE.random(ctx, n_vars, 1234 + n_vars).free()
        MLE.random(ctx, 12, 99).free()
        a, b = _rand(field, 31, la), _rand(field, 32, lb)
        A = UP.new(ctx, a)   # takes the block the random table left
        B = UP.new(ctx, b)
        assert _ints(field, (A * B).coefficients()) == schoolbook(field, _ints(field, a), _ints(field, b))
    ctx.close()


_CHILD = r"""
import hashlib, sys
sys.path.insert(0, {root!r})
import zk_amd
from oracle import binding as orc
field = {field}
ctx = zk_amd.Context(field, 0)
h = hashlib.sha256()
for n, (la, lb) in enumerate({shapes!r}):
    a = orc.fill_random(field, 40 + n, la)
    A = zk_amd.UnivariatePolynomial.new(ctx, a)
    B = A if lb is None else zk_amd.UnivariatePolynomial.new(ctx, orc.fill_random(field, 80 + n, lb))
    h.update((A * B).coefficients().tobytes())
print("DIGEST", h.hexdigest())
"""


@pytest.mark.parametrize("field", FIELDS)
def test_direct_and_ntt_paths_give_the_same_bytes(field):
    shapes = [(40, 300), (33, 5000), (100, 1000), (257, 257), (1, 4096), (3, 1 << 16), (300, None), (129, 128), (2, 200)]
    digests = {}
    for setting in ("0", str(1 << 40), None):   # never (N < 2^8 stays direct), always, the default
        env = dict(os.environ)
        env.pop("ZK_UPOLY_DIRECT_MAX", None)
        if setting is not None:
            env["ZK_UPOLY_DIRECT_MAX"] = setting
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, field=field, shapes=shapes)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        digests[setting] = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")]
    assert digests["0"] == digests[str(1 << 40)] == digests[None] and digests["0"]
    # and the bytes are the schoolbook product's
    h = hashlib.sha256()
    for n, (la, lb) in enumerate(shapes):
        a = orc.fill_random(field, 40 + n, la)
        b = a if lb is None else orc.fill_random(field, 80 + n, lb)
        h.update(_elems(field, schoolbook(field, _ints(field, a), _ints(field, b))).tobytes())
    assert digests["0"] == ["DIGEST " + h.hexdigest()]


def test_structured_products_on_the_default_path(fctx):
    """tests/upoly_structured_check.py under the shipped path selection: products whose transforms hold exact zeros (1 - x^m,
    (1 + x^(N/2)) b, the squares of 1 + x^(N/2) and 1 - x^(N/4)) and all-(p-1) operands, each against its closed form"""
    import upoly_structured_check as usc

    field, ctx = fctx
    assert usc.run(field, ctx) == 20


@pytest.mark.parametrize("setting", ["0", str(1 << 40)], ids=["ntt", "direct"])
@pytest.mark.parametrize("field", FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def test_structured_products_on_both_forced_paths(field, setting):
    """the same cases with every product of 2^8 points and more on the fused NTT passes (kNttPadLoad, kNttMulStore, kNttSqrStore,
    kNttTruncStore on exact zeros), and with every product on the direct kernel (fe_mul_tt_lazy with fe_add2 over all-(p-1)
    operands); one fresh child each, forced as test_direct_and_ntt_paths_give_the_same_bytes forces them"""
    env = dict(os.environ, ZK_UPOLY_DIRECT_MAX=setting)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "upoly_structured_check.py"), str(field)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"upoly structured ok: 20 products (ZK_UPOLY_DIRECT_MAX={setting})" in r.stdout, r.stdout[-2000:]


def test_evaluate_against_horner(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    xs = [0, 1, p - 1, random.Random(field).randrange(p)]
    lens = [0, 1, 2, 15, 17, 255, 257, 4095, 4096, 4097, 8191, 8193]
    if field == zk_amd.BLS12_381_FR:
        lens += [(1 << 16) - 1, (1 << 16) + 1, (1 << 20) + 1]
    for n, ln in enumerate(lens):
        co = _rand(field, 700 + n, ln)
        h = UP.new(ctx, co)
        ci = _ints(field, co)
        for x in xs if ln <= 8193 else xs[2:]:
            assert orc.to_int(field, h.evaluate(orc.from_int(field, x))) == horner(field, ci, x), (ln, x)
        assert np.array_equal(h.coefficients(), co)   # evaluate leaves its input alone


def test_evaluate_2p24():
    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    p = orc.modulus(field)
    for ln in ((1 << 24) - 1, 1 << 24):
        co = _rand(field, 800 + ln, ln)
        h = UP.new(ctx, co)
        ev = lambda x: orc.to_int(field, h.evaluate(orc.from_int(field, x)))  # noqa: E731
        assert ev(0) == orc.to_int(field, co[0])
        assert ev(1) == orc.to_int(field, orc.sum_elems(field, co))
        assert ev(p - 1) == (orc.to_int(field, orc.sum_elems(field, co[0::2])) - orc.to_int(field, orc.sum_elems(field, co[1::2]))) % p
        if ln == 1 << 24:
            x = random.Random(5).randrange(p)
            assert ev(x) == horner(field, _ints(field, co), x)
    ctx.close()


def test_error_table():
    field = zk_amd.BN254_FR
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    a = UP.new(ctx, _rand(field, 1, 8))
    b_other = UP.new(other, _rand(field, 2, 8))
    x = np.zeros(4, dtype=np.uint64)
    out = np.zeros((16, 4), dtype=np.uint64)
    h = c.c_void_p()
    u64p = c.POINTER(c.c_uint64)
    p = lambda v: v.ctypes.data_as(u64p)  # noqa: E731
    BAD, MISMATCH, UNSUP = -20, -26, -25
    assert lib.zk_upoly_mul(ctx._h, a._h, None, c.byref(h)) == BAD
    assert lib.zk_upoly_mul(ctx._h, a._h, a._h, None) == BAD
    assert lib.zk_upoly_mul(None, a._h, a._h, c.byref(h)) == BAD
    assert lib.zk_upoly_evaluate(ctx._h, a._h, None, p(x)) == BAD
    assert lib.zk_upoly_evaluate(ctx._h, None, p(x), p(x)) == BAD
    assert lib.zk_upoly_upload(ctx._h, None, 3, c.byref(h)) == BAD
    assert lib.zk_upoly_download(ctx._h, a._h, None) == BAD
    assert lib.zk_upoly_len(a._h, None) == BAD
    assert lib.zk_upoly_mul_host(ctx._h, None, 3, p(out), 3, p(out)) == BAD
    assert lib.zk_upoly_mul_host(ctx._h, p(out), 3, p(out), 3, None) == BAD
    assert lib.zk_upoly_mul(ctx._h, a._h, b_other._h, c.byref(h)) == MISMATCH
    assert lib.zk_upoly_mul(other._h, a._h, b_other._h, c.byref(h)) == MISMATCH
    assert lib.zk_upoly_evaluate(other._h, a._h, p(x), p(x)) == MISMATCH
    assert lib.zk_upoly_download(other._h, a._h, p(out)) == MISMATCH
    assert lib.zk_upoly_free(other._h, a._h) == MISMATCH
    assert lib.zk_upoly_free(None, a._h) == BAD
    # the length rule, checked before the (short) inputs are read: N = 2^ceil(log2(la + lb - 1)) past 2^two_adicity
    s = zk_amd.two_adicity(field)
    big = (1 << (s - 1)) + 1
    assert lib.zk_upoly_mul_host(ctx._h, p(out), big, p(out), big, p(out)) == UNSUP
    assert lib.zk_upoly_mul_host(ctx._h, p(out), 1 << 41, p(out), 1, p(out)) == UNSUP
    # an empty operand: nothing is written, out may be NULL
    assert lib.zk_upoly_mul_host(ctx._h, p(out), 0, p(out), 3, None) == 0
    with pytest.raises(ZkError) as e:
        a * b_other
    assert e.value.code == MISMATCH
    a.free()
    b_other.free()
    ctx.close()
    other.close()


def test_cpp_host_mirror_kats_and_2p20_product(tmp_path):
    """tests/cpp/test_upoly.cpp over zk.hpp: the KATs and one 2^20 product against values this test passes in"""
    field = zk_amd.BN254_FR
    exe = str(tmp_path / "test_upoly")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_upoly.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    la, lb = 1 << 19, (1 << 19) - 5
    a, b = _rand(field, 901, la), _rand(field, 902, lb)
    want = _oracle_product(field, a, b)
    for name, arr in (("a", a), ("b", b), ("c", want)):
        arr.astype("<u8").tofile(str(tmp_path / f"{name}.bin"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: upoly host tests passed" in r.stdout
