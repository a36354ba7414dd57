"""zk_mle_batch_inverse, zk_upoly_batch_inverse, zk_mle_prefix_product and zk_batch_inverse_host on the device.  The reference has
neither: tests/batch_inverse_ref.py is the definition.  The one-launch kernel and the three launches in child processes under
ZK_BATCH_INV_ONE_LAUNCH_MAX, bit for bit against pow(x, p - 2, p) on every boundary length and zero placement; table handles in and
out of place over stale pool blocks, more chunks than the middle workgroup has threads (by the product property on the CPU oracle),
the running products, the error table, the host form, the measurement hook and the C++ mirror in the parent."""
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
from zk_amd._lib import c, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_inverse_ref as ref  # noqa: E402
from batch_inverse_check import FIELD_IDS, SETTINGS, SWITCH, digest  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "batch_inverse_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BAD, MISMATCH, UNSUP = -20, -26, -25
C = ref.CHUNK


@pytest.fixture(scope="module")
def children():
    """{setting: {(field id, case): (digest with count, count, digest without count)}}: one child process per switch setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"batch inverse {setting} ok" in r.stdout
        lines = [ln.split() for ln in r.stdout.splitlines()]
        out[setting] = {(ln[1], ln[2]): (ln[3], int(ln[4]), ln[5]) for ln in lines if ln and ln[0] == "DIGEST"}
    return out


@pytest.fixture(scope="module")
def expected():
    """{(field id, case): (digest, zeros)} from the big-int definition, computed once"""
    out = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        cache = {}
        for n in ref.LENGTHS:
            for name, vals, shift in ref.cases(p, fi, n, worst_case_values):
                inv, zeros = ref.batch_inverse(vals, shift, p, cache)
                out[(FIELD_IDS[fi], f"n{n}_{name}")] = (digest(orc.from_ints(field, inv)), zeros)
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_length_and_zero_placement_on_every_path(children, expected, setting):
    """lengths 0 .. 2 CHUNK + 1 through zk_upoly_batch_inverse, with and without a shift, every zero placement, with and without the
    count: the bytes and the count of the definition, on the one-launch kernel, the three launches and the default"""
    got = children[setting]
    assert len(expected) == 3 * len(ref.LENGTHS) * 11 and set(got) == set(expected)
    for key, (want, zeros) in expected.items():
        assert got[key][0] == want, (setting, key)
        assert got[key][1] == zeros, (setting, key, got[key][1], zeros)
        assert got[key][2] == want, (setting, key, "without the count")
    # the placements did plant what they say (a count of zero everywhere would pass nothing)
    assert expected[("bn254", f"n{2 * C + 1}_all_zero")][1] == 2 * C + 1 and expected[("bn254", f"n{C}_zero_by_shift_only")][1] == 4


@pytest.fixture(params=range(3), ids=FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def _mle_round(ctx, field, p, fi, cache):
    for n_vars in ref.MLE_VARS:
        n = 1 << n_vars
        for name, vals, shift in ref.cases(p, fi, n, worst_case_values):
            if name not in ("random", "random_shift", "chunk_first_and_last", "zero_by_shift_only"):
                continue
            src = orc.from_ints(field, vals)
            sh = orc.from_int(field, shift) if shift else None
            want, zeros = ref.batch_inverse(vals, shift, p, cache)
            want = orc.from_ints(field, want)
            t = MLE.new(ctx, n_vars, src)
            out, got_zeros = t.batch_inverse(shift=sh, count_zeros=True)   # out of place, a new table
            assert got_zeros == zeros and np.array_equal(out.evaluation_slice(), want), (n_vars, name)
            assert np.array_equal(t.evaluation_slice(), src), (n_vars, name, "the source changed")
            other = MLE.random(ctx, n_vars, 3)
            assert t.batch_inverse(shift=sh, out=other) is other and np.array_equal(other.evaluation_slice(), want)   # ... a given one, no count
            same, got_zeros = t.batch_inverse(shift=sh, out=t, count_zeros=True)   # in place
            assert same is t and got_zeros == zeros and np.array_equal(t.evaluation_slice(), want), (n_vars, name, "in place")


def test_table_handles_in_and_out_of_place_and_over_stale_pool(fctx):
    fi, field, ctx = fctx
    p = orc.modulus(field)
    cache = {}
    _mle_round(ctx, field, p, fi, cache)
    # a large handle of non-zero data goes back to the pool: the scratch of the next calls is cut from it, and is not zero
    big = MLE.random(ctx, 16, 9)
    for n_vars in (0, 1, 3, 5, 6, 10, 11, 12):
        MLE.random(ctx, n_vars, 40 + n_vars).free()
    big.free()
    _mle_round(ctx, field, p, fi, cache)


def _pad_one(field, a, n_vars):
    out = np.tile(orc.from_int(field, 1), (1 << n_vars, 1))
    out[: a.shape[0]] = a
    return out


def test_more_chunks_than_the_middle_workgroup_has_threads():
    """256 CHUNK + 1 elements through the vector entry and 2^(log2(256 CHUNK) + 1) through the table entry: the middle launch's threads
    take more than one chunk each.  Checked by in[i] * out[i] == 1 (0 at the planted zeros) on the CPU oracle: the inverse is unique."""
    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    one, zero = orc.from_int(field, 1), np.zeros(4, dtype=np.uint64)
    for kind, n in (("upoly", 256 * C + 1), ("mle", 512 * C)):
        n_vars = (n - 1).bit_length()
        src = orc.fill_random(field, 0xBA7C + n % 7, n)
        planted = [C - 1, C, 200 * C]   # the last element of a chunk, the first of the next, the first of one deep in the second round of the middle launch
        assert not (src == 0).all(axis=1).any()
        src[planted] = 0
        if kind == "upoly":
            out, zeros = UP.new(ctx, src).batch_inverse(count_zeros=True)
            got = out.coefficients()
        else:
            t = MLE.new(ctx, n_vars, src)
            out, zeros = t.batch_inverse(out=t, count_zeros=True)
            got = out.evaluation_slice()
        assert zeros == len(planted), (kind, zeros)
        prod = orc.prod_reduce(field, n_vars, [_pad_one(field, src, n_vars), _pad_one(field, got, n_vars)])
        want = np.tile(one, (1 << n_vars, 1))
        want[planted] = zero
        bad = np.flatnonzero((prod != want).any(axis=1))
        assert bad.size == 0, (kind, bad[:8])
        assert not got[planted].any()
    ctx.close()


def test_prefix_product_small_sizes_against_the_definition(fctx):
    fi, field, ctx = fctx
    p = orc.modulus(field)
    for n_vars in (0, 1, 6, 11, 12, 13):   # 2^12 elements are one chunk of the scan, 2^13 two
        n = 1 << n_vars
        base = ref.base_values(p, fi, n, worst_case_values)
        with_zero = list(base)
        with_zero[n // 2] = 0
        for vals in (base, with_zero):
            src = orc.from_ints(field, vals)
            for inclusive in (False, True):
                want, total = ref.prefix_product(vals, inclusive, p)
                want = orc.from_ints(field, want)
                t = MLE.new(ctx, n_vars, src)
                out, got_total = t.prefix_product(inclusive=inclusive, want_total=True)
                assert np.array_equal(out.evaluation_slice(), want), (n_vars, inclusive)
                assert orc.to_int(field, got_total) == total, (n_vars, inclusive)
                assert np.array_equal(t.evaluation_slice(), src)
                quiet = t.prefix_product(inclusive=inclusive)   # no total: no host wait
                assert quiet == out
                same = t.prefix_product(inclusive=inclusive, out=t)   # in place
                assert same is t and np.array_equal(t.evaluation_slice(), want), (n_vars, inclusive, "in place")
            if vals is with_zero and n > 1:
                assert total == 0 and not want[n // 2 + 1:].any()   # everything after the zero is zero


def test_prefix_product_large_by_the_recurrence():
    """2^21 elements (512 chunks of the scan: two per thread of its middle launch): exclusive[0] = 1, exclusive[1:] = (exclusive * t)[:-1],
    inclusive = exclusive * t, total = its last element -- the products on the CPU oracle"""
    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    n_vars = 21
    src = orc.fill_random(field, 0x9F1, 1 << n_vars)
    t = MLE.new(ctx, n_vars, src)
    excl = t.prefix_product()
    incl, total = t.prefix_product(inclusive=True, want_total=True)
    e, i = excl.evaluation_slice(), incl.evaluation_slice()
    prod = orc.prod_reduce(field, n_vars, [e, src])
    assert np.array_equal(e[0], orc.from_int(field, 1))
    assert np.array_equal(e[1:], prod[:-1])
    assert np.array_equal(i, prod)
    assert np.array_equal(total, prod[-1])
    in_place, total2 = t.prefix_product(out=t, want_total=True)
    assert in_place == excl and np.array_equal(total2, total)
    ctx.close()


def test_inverse_and_running_product_commute(fctx):
    """for a table without zeros, prefix_product(batch_inverse(t)) == batch_inverse(prefix_product(t)) element by element"""
    fi, field, ctx = fctx
    n_vars = ref.LOG_CHUNK + 1
    t = MLE.new(ctx, n_vars, orc.from_ints(field, ref.base_values(orc.modulus(field), fi, 1 << n_vars, worst_case_values)))
    for inclusive in (False, True):
        a = t.batch_inverse().prefix_product(inclusive=inclusive)
        b, zeros = t.prefix_product(inclusive=inclusive).batch_inverse(count_zeros=True)
        assert zeros == 0
        eq = c.c_int32()
        assert lib.zk_mle_equal(ctx._h, a._h, b._h, c.byref(eq)) == 0 and eq.value == 1, inclusive


def test_host_form(fctx):
    fi, field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(77 + fi)
    for n in (1, 5, C + 3):
        vals = [rng.randrange(p) for _ in range(n)]
        vals[n // 2] = 0
        shift = rng.randrange(1, p)
        for s in (0, shift):
            want, zeros = ref.batch_inverse(vals, s, p)
            got, got_zeros = zk_amd.batch_inverse_host(ctx, orc.from_ints(field, vals), orc.from_int(field, s) if s else None)
            assert got_zeros == zeros and orc.to_ints(field, got) == want, (n, bool(s))
    got, zeros = zk_amd.batch_inverse_host(ctx, np.zeros((0, 4), dtype=np.uint64))   # n = 0 with NULL buffers
    assert got.shape == (0, 4) and zeros == 0
    z = c.c_uint64(7)
    assert lib.zk_batch_inverse_host(ctx._h, None, 0, None, None, c.byref(z)) == 0 and z.value == 0
    assert lib.zk_batch_inverse_host(ctx._h, None, 0, None, None, None) == 0
    buf = orc.from_ints(field, [3, 0, 4])   # in place, no count
    bp = buf.ctypes.data_as(c.POINTER(c.c_uint64))
    assert lib.zk_batch_inverse_host(ctx._h, bp, 3, None, bp, None) == 0
    assert orc.to_ints(field, buf) == ref.batch_inverse([3, 0, 4], 0, p)[0]


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    t, o, small = MLE.random(ctx, 6, 1), MLE.random(ctx, 6, 2), MLE.random(ctx, 5, 3)
    t_other = MLE.random(other, 6, 1)
    v = UP.new(ctx, orc.fill_random(field, 4, 9))
    v_other = UP.new(other, orc.fill_random(field, 4, 9))
    before = o.evaluation_slice().copy()
    h, z, ms = c.c_void_p(), c.c_uint64(99), c.c_double(-1.0)
    tot = np.full(4, 7, dtype=np.uint64)
    tp = tot.ctypes.data_as(c.POINTER(c.c_uint64))
    # nulls
    assert lib.zk_mle_batch_inverse(None, t._h, None, o._h, c.byref(z)) == BAD
    assert lib.zk_mle_batch_inverse(ctx._h, None, None, o._h, c.byref(z)) == BAD
    assert lib.zk_mle_batch_inverse(ctx._h, t._h, None, None, c.byref(z)) == BAD
    assert lib.zk_upoly_batch_inverse(None, v._h, None, c.byref(h), c.byref(z)) == BAD
    assert lib.zk_upoly_batch_inverse(ctx._h, None, None, c.byref(h), c.byref(z)) == BAD
    assert lib.zk_upoly_batch_inverse(ctx._h, v._h, None, None, c.byref(z)) == BAD
    assert lib.zk_mle_prefix_product(None, t._h, 0, o._h, tp) == BAD
    assert lib.zk_mle_prefix_product(ctx._h, None, 0, o._h, tp) == BAD
    assert lib.zk_mle_prefix_product(ctx._h, t._h, 0, None, tp) == BAD
    assert lib.zk_batch_inverse_host(None, tp, 1, None, tp, None) == BAD
    assert lib.zk_batch_inverse_host(ctx._h, None, 1, None, tp, None) == BAD
    assert lib.zk_batch_inverse_host(ctx._h, tp, 1, None, None, None) == BAD
    assert lib.zk_batch_inverse_host(ctx._h, tp, (1 << 40) + 1, None, tp, None) == UNSUP   # before anything is read
    # another context's handle
    assert lib.zk_mle_batch_inverse(ctx._h, t_other._h, None, o._h, c.byref(z)) == MISMATCH
    assert lib.zk_mle_batch_inverse(ctx._h, t._h, None, t_other._h, c.byref(z)) == MISMATCH
    assert lib.zk_mle_batch_inverse(other._h, t._h, None, o._h, c.byref(z)) == MISMATCH
    assert lib.zk_upoly_batch_inverse(ctx._h, v_other._h, None, c.byref(h), c.byref(z)) == MISMATCH
    assert lib.zk_upoly_batch_inverse(other._h, v._h, None, c.byref(h), c.byref(z)) == MISMATCH
    assert lib.zk_mle_prefix_product(ctx._h, t_other._h, 0, o._h, tp) == MISMATCH
    assert lib.zk_mle_prefix_product(ctx._h, t._h, 1, t_other._h, tp) == MISMATCH
    assert lib.zk_bench_batch_inverse(ctx._h, t_other._h, o._h, 0, 1, c.byref(ms)) == MISMATCH
    assert lib.zk_bench_batch_inverse(ctx._h, t._h, t_other._h, 0, 1, c.byref(ms)) == MISMATCH
    # a wrong-size out
    assert lib.zk_mle_batch_inverse(ctx._h, t._h, None, small._h, c.byref(z)) == BAD
    assert lib.zk_mle_batch_inverse(ctx._h, small._h, None, o._h, None) == BAD
    assert lib.zk_mle_prefix_product(ctx._h, t._h, 0, small._h, tp) == BAD
    assert lib.zk_bench_batch_inverse(ctx._h, t._h, small._h, 0, 1, c.byref(ms)) == BAD
    # the measurement hook's own arguments
    assert lib.zk_bench_batch_inverse(None, t._h, o._h, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_batch_inverse(ctx._h, None, o._h, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_batch_inverse(ctx._h, t._h, None, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_batch_inverse(ctx._h, t._h, o._h, 0, 1, None) == BAD
    assert lib.zk_bench_batch_inverse(ctx._h, t._h, o._h, 0, 0, c.byref(ms)) == BAD
    assert lib.zk_bench_batch_inverse(ctx._h, t._h, o._h, 4, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_batch_inverse(ctx._h, t._h, o._h, -1, 1, c.byref(ms)) == BAD
    big, big_o = MLE.random(ctx, ref.LOG_CHUNK + 1, 5), MLE.alloc(ctx, ref.LOG_CHUNK + 1)
    assert lib.zk_bench_batch_inverse(ctx._h, big._h, big_o._h, 1, 1, c.byref(ms)) == UNSUP   # more than a chunk cannot take one launch
    # nothing was returned or written by any of them
    assert not h.value and z.value == 99 and ms.value == -1.0 and (tot == 7).all()
    assert np.array_equal(o.evaluation_slice(), before)
    # every path of the hook gives a time, and leaves the inverse (the running product on path 3) in out
    for path, tab, out in ((0, t, o), (1, t, o), (2, t, o), (3, t, o), (0, big, big_o), (2, big, big_o), (3, big, big_o)):
        ms.value = -1.0
        assert lib.zk_bench_batch_inverse(ctx._h, tab._h, out._h, path, 2, c.byref(ms)) == 0 and ms.value > 0, path
        assert out == (tab.prefix_product() if path == 3 else tab.batch_inverse()), path
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_batch_inverse.cpp over zk.hpp: x * (1 / x) = 1 through the C++ mirror, zeros, shift, in place, running products"""
    exe = str(tmp_path / "test_batch_inverse")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_batch_inverse.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: batch inverse host tests passed" in r.stdout
