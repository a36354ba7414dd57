"""Dense coefficient-form multilinear polynomials on the device (zk_cmle_*; coefficient_form.rs :39-69 evaluate_slice, :131-139 to_bytes,
:200-216 interpolate, :340-347 to_evaluation_form): byte-identical to the Python restatement (tests/cmle_ref.py) at small sizes and for
every length 0..70, round trips through the oracle-pinned coeff_to_evaluation paths up to 2^24, evaluate against the MLE evaluator (the
multilinear extension is unique), inclusion-exclusion at 2^24, to_bytes against the model and a numpy rebuild, and the error table."""
import hashlib
import os
import random
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import CoeffMultilinearPolynomial as CMLE
from zk_amd import DeviceCoeffMultilinear as DC
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import ZkError
from zk_amd._lib import c, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cmle_ref import evaluate_slice, interpolate_fast, to_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
EVAL_LEN, EVAL_ASSIGNMENT, BAD_ARG, CONTEXT_MISMATCH = -1, -12, -20, -26


@pytest.fixture(params=FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def fctx(request):
    ctx = zk_amd.Context(request.param, 0)
    yield request.param, ctx
    ctx.close()


@pytest.fixture
def bn():
    ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
    yield zk_amd.BN254_FR, ctx
    ctx.close()


def _rand(field, seed, n):
    return orc.fill_random(field, seed, n) if n else np.zeros((0, 4), dtype=np.uint64)


def _model(field, table):
    """interpolate_fast over canonical ints -> (n_vars, Montgomery elements)"""
    n, dense = interpolate_fast(orc.to_ints(field, table), orc.modulus(field))
    return n, (orc.from_ints(field, dense) if dense else np.zeros((0, 4), dtype=np.uint64))


def _mobius_keys(field, table, n):
    """the model for larger n, vectorised over object arrays: Moebius of the table, then bit reversal into key order"""
    p = orc.modulus(field)
    t = np.array(orc.to_ints(field, table), dtype=object)
    for b in range(n):
        v = t.reshape(-1, 2, 1 << b)
        v[:, 1, :] = (v[:, 1, :] - v[:, 0, :]) % p
    rev = np.array([int(format(k, f"0{n}b")[::-1], 2) for k in range(1 << n)])
    return orc.from_ints(field, [int(x) for x in t[rev]])


def _dense_terms(coeffs):
    return np.arange(coeffs.shape[0], dtype=np.uint64), np.ascontiguousarray(coeffs)


def _coeff_to_eval(ctx, n, coeffs):
    keys, co = _dense_terms(coeffs)
    return _zk_coeff_to_evaluation(ctx, n, keys, co)


def _zk_coeff_to_evaluation(ctx, n, keys, coeffs):
    h = c.c_void_p()
    rc = lib.zk_coeff_to_evaluation(ctx._h, n, keys.ctypes.data_as(c.POINTER(c.c_uint64)), coeffs.ctypes.data_as(c.POINTER(c.c_uint64)),
                                     keys.size, c.byref(h))
    assert rc == 0, rc
    return MLE(ctx, h)


def test_interpolate_small_matches_model(fctx):
    field, ctx = fctx
    for n in range(0, 15):
        table = _rand(field, 0xC0 + n, 1 << n)
        want_n, want = _model(field, table)
        assert want_n == max(n, 1)
        d = DC.interpolate(ctx, MLE.new(ctx, n, table))
        assert d.n_vars() == want_n and np.array_equal(d.coefficients(), want), n
        hn, host = zk_amd.cmle_interpolate_host(ctx, table)
        assert hn == want_n and np.array_equal(host, want), n
        assert np.array_equal(table, MLE.new(ctx, n, table).evaluation_slice())   # the table is left intact


def test_interpolate_every_length_matches_model(fctx):
    field, ctx = fctx
    for length in range(0, 71):
        vals = _rand(field, 0x1E0 + length, length)
        want_n, want = _model(field, vals)
        hn, host = zk_amd.cmle_interpolate_host(ctx, vals)
        assert hn == want_n and host.shape == want.shape and np.array_equal(host, want), length
        poly = CMLE.interpolate(ctx, vals)
        assert poly.n_vars() == want_n and sorted(poly.coefficients) == list(range(want.shape[0]))   # every key, zeros included
        if length:
            assert np.array_equal(DC.interpolate(ctx, vals).coefficients(), want)
    p = orc.modulus(field)
    assert orc.to_ints(field, zk_amd.cmle_interpolate_host(ctx, orc.from_ints(field, [2, 4, 8, 3]))[1]) == [2, 6, 2, p - 7]   # the KAT
    assert orc.to_ints(field, zk_amd.cmle_interpolate_host(ctx, orc.from_ints(field, [9]))[1]) == [9, p - 9]


@pytest.mark.parametrize("n", [16, 18])
def test_interpolate_bn254_larger(bn, n):
    field, ctx = bn
    table = _rand(field, 0x16 + n, 1 << n)
    d = DC.interpolate(ctx, MLE.new(ctx, n, table))
    assert np.array_equal(d.coefficients(), _mobius_keys(field, table, n))


def test_round_trip_through_oracle(fctx):
    field, ctx = fctx
    for n in list(range(1, 13)) + [14]:   # the oracle's transform is quadratic in the table: 2^18 takes 18 s
        table = _rand(field, 0x2A0 + n, 1 << n)
        co = DC.interpolate(ctx, MLE.new(ctx, n, table)).coefficients()
        keys, cc = _dense_terms(co)
        assert np.array_equal(orc.coeff_to_evaluation(field, n, keys, cc), table), n


def _round_trip(ctx, n, seed):
    t = MLE.random(ctx, n, seed)
    d = DC.interpolate(ctx, t)
    assert _coeff_to_eval(ctx, n, d.coefficients()) == t   # the downloaded coefficients as a 2^n-term list
    assert d.to_evaluation_form() == t


def test_round_trip_through_zk_coeff_to_evaluation_2p20(fctx):
    field, ctx = fctx
    _round_trip(ctx, 20, 0x2414)


def test_round_trip_through_zk_coeff_to_evaluation_2p24_bn254(bn):
    _round_trip(bn[1], 24, 0x2418)


def test_to_evaluation_matches_zk_coeff_to_evaluation(fctx):
    field, ctx = fctx
    for n in list(range(1, 15)) + [20]:
        co = _rand(field, 0x3B0 + n, 1 << n)
        got = DC.upload(ctx, n, co).to_evaluation_form()
        assert got == _coeff_to_eval(ctx, n, co), n
    with pytest.raises(ZkError) as e:
        DC.upload(ctx, 0, _rand(field, 1, 1)).to_evaluation_form()
    assert e.value.code == EVAL_LEN


def test_to_evaluation_bn254_2p24(bn):
    field, ctx = bn
    n = 24
    d = DC.upload(ctx, n, MLE.random(ctx, n, 0x3C24).evaluation_slice())
    assert d.to_evaluation_form() == _coeff_to_eval(ctx, n, d.coefficients())


def _points(field, n, seed):
    rng = random.Random(seed)
    p = orc.modulus(field)
    specials = [0, 1, p - 1]
    pts = [[specials[rng.randrange(3)] if rng.random() < 0.5 else rng.randrange(p) for _ in range(n)],
           [p - 1] * n, [0] * n, [1] * n, [rng.randrange(p) for _ in range(n)]]
    return [orc.from_ints(field, q) for q in pts]


def test_evaluate_matches_mle_evaluate(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    for n in list(range(1, 15)) + [20]:
        table = _rand(field, 0x4C0 + n, 1 << n)
        t = MLE.new(ctx, n, table)
        d = DC.interpolate(ctx, t)
        dense = orc.to_ints(field, d.coefficients()) if n <= 10 else None
        for k, pt in enumerate(_points(field, n, n)):
            got = d.evaluate_slice(pt)
            assert np.array_equal(got, t.evaluate(pt)), (n, k)
            if dense is not None:
                assert orc.to_int(field, got) == evaluate_slice(n, dense, orc.to_ints(field, pt), p)
        extra = np.concatenate([pt, _rand(field, 99, 3)])
        assert np.array_equal(d.evaluate_slice(extra), t.evaluate(pt))   # assignments past n_vars are ignored
        with pytest.raises(ZkError) as e:
            d.evaluate_slice(pt[:-1])
        assert e.value.code == EVAL_ASSIGNMENT and str(e.value) == "evaluate requires an assignment for every variable"
    d0 = DC.upload(ctx, 0, orc.from_ints(field, [42]))
    assert orc.to_int(field, d0.evaluate_slice(np.zeros((0, 4), dtype=np.uint64))) == 42   # n_vars 0: the coefficient of key 0


def test_2p24_bn254_evaluate_inclusion_exclusion_and_to_bytes(bn):
    field, ctx = bn
    n = 24
    p = orc.modulus(field)
    t = MLE.random(ctx, n, 0x5E24)
    d = DC.interpolate(ctx, t)
    for k, pt in enumerate(_points(field, n, 24)):
        assert np.array_equal(d.evaluate_slice(pt), t.evaluate(pt)), k
    table = t.evaluation_slice()
    co = d.coefficients()
    rng = random.Random(3)
    keys = [0, 1 << 23, 1, 3, (1 << 23) | (1 << 5) | 1]
    while len(keys) < 24:
        keys.append(sum(1 << v for v in rng.sample(range(n), rng.randrange(1, 4))))
    for key in keys:   # coefficient of key k = sum over subsets S of k of (-1)^{|k|-|S|} T[index of S]
        vs = [v for v in range(n) if key >> v & 1]
        acc = 0
        for mask in range(1 << len(vs)):
            idx = sum(1 << (n - 1 - vs[i]) for i in range(len(vs)) if mask >> i & 1)
            sign = -1 if (len(vs) - bin(mask).count("1")) & 1 else 1
            acc += sign * orc.to_int(field, table[idx])
        assert orc.to_int(field, co[key]) == acc % p, key
    # to_bytes against a rebuild: 32-byte canonical elements from the oracle-pinned MLE serialiser, keys by numpy
    got = d.to_bytes_array()
    elems = MLE.new(ctx, n, co).to_bytes_array().reshape(-1, 32)
    rec = np.empty((1 << n, 40), dtype=np.uint8)
    rec[:, :8] = np.arange(1 << n, dtype=">u8").view(np.uint8).reshape(-1, 8)
    rec[:, 8:] = elems
    want = hashlib.sha256(n.to_bytes(4, "big") + rec.tobytes()).hexdigest()
    assert hashlib.sha256(got.tobytes()).hexdigest() == want


def test_to_bytes_matches_model(fctx):
    field, ctx = fctx
    for n in range(0, 13):
        co = _rand(field, 0x6B0 + n, 1 << n)
        assert DC.upload(ctx, n, co).to_bytes() == to_bytes(n, orc.to_ints(field, co)), n


def test_error_table(fctx):
    field, ctx = fctx
    h = c.c_void_p()
    nv = c.c_uint64()
    out = np.zeros(4, dtype=np.uint64)
    u64 = lambda a: a.ctypes.data_as(c.POINTER(c.c_uint64))  # noqa: E731
    vals = _rand(field, 7, 8)
    assert lib.zk_cmle_upload(ctx._h, 3, u64(vals), 7, c.byref(h)) == EVAL_LEN
    assert lib.zk_cmle_upload(ctx._h, 2, u64(vals), 8, c.byref(h)) == EVAL_LEN
    assert lib.zk_cmle_upload(ctx._h, 3, None, 8, c.byref(h)) == BAD_ARG
    assert lib.zk_cmle_upload(ctx._h, 41, u64(vals), 1 << 41, c.byref(h)) == -25   # size limit, before anything is read
    assert lib.zk_cmle_interpolate_host(ctx._h, u64(vals), (1 << 40) + 1, c.byref(nv), u64(out)) == -25
    assert lib.zk_cmle_interpolate_host(ctx._h, None, 0, c.byref(nv), None) == 0 and nv.value == 0   # empty: no variable, no key
    assert lib.zk_cmle_interpolate_host(ctx._h, u64(vals), 8, c.byref(nv), None) == BAD_ARG
    d = DC.upload(ctx, 3, vals)
    t = MLE.new(ctx, 3, vals)
    assert lib.zk_cmle_interpolate(ctx._h, None, c.byref(h)) == BAD_ARG
    assert lib.zk_cmle_interpolate(ctx._h, t._h, None) == BAD_ARG
    assert lib.zk_cmle_to_evaluation(ctx._h, d._h, None) == BAD_ARG
    assert lib.zk_cmle_evaluate(ctx._h, d._h, None, 3, u64(out)) == BAD_ARG
    assert lib.zk_cmle_to_bytes(ctx._h, d._h, None) == BAD_ARG
    assert lib.zk_cmle_download(ctx._h, d._h, None) == BAD_ARG
    other = zk_amd.Context(field, 0)
    try:
        buf = np.zeros(4 + 40 * 8, dtype=np.uint8)
        assert lib.zk_cmle_interpolate(other._h, t._h, c.byref(h)) == CONTEXT_MISMATCH
        assert lib.zk_cmle_to_evaluation(other._h, d._h, c.byref(h)) == CONTEXT_MISMATCH
        assert lib.zk_cmle_evaluate(other._h, d._h, u64(vals), 3, u64(out)) == CONTEXT_MISMATCH
        assert lib.zk_cmle_to_bytes(other._h, d._h, buf.ctypes.data_as(c.POINTER(c.c_uint8))) == CONTEXT_MISMATCH
        assert lib.zk_cmle_download(other._h, d._h, u64(np.zeros((8, 4), dtype=np.uint64))) == CONTEXT_MISMATCH
        assert lib.zk_cmle_free(other._h, d._h) == CONTEXT_MISMATCH
    finally:
        other.close()
    with pytest.raises(ValueError):
        DC.interpolate(ctx, np.zeros((0, 4), dtype=np.uint64))
    assert CMLE.interpolate(ctx, np.zeros((0, 4), dtype=np.uint64)).n_vars() == 0


def test_bench_hook_runs(bn):
    field, ctx = bn
    t = MLE.random(ctx, 12, 5)
    d = DC.interpolate(ctx, t)
    pt = _rand(field, 6, 12)
    for op in range(3):
        assert d.bench(op, table=t, point=pt, reps=2) > 0


def test_cpp_mirror(tmp_path):
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_cmle")
    lib_dir = os.path.join(root, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "test_cmle.cpp"), "-L" + lib_dir,
                    "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_cmle: ok" in r.stdout, r.stdout + r.stderr
