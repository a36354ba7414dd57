"""zk_upoly_divrem and zk_upoly_inverse_series on the device.  The reference has no division: tests/divrem_ref.py is the definition.
The direct kernel, the Newton path and the linear-divisor scan in child processes under ZK_UPOLY_DIVREM_DIRECT_MAX and
ZK_UPOLY_DIVREM_LINEAR, bit for bit against big-int schoolbook division on the small cases and by exact construction on the large
ones; aliasing, skipped results, empty operands, stale pool blocks, the series inverse, the error table and the C++ mirror in the
parent."""
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
from divrem_check import FIELD_IDS, LARGE, SETTINGS, digest, small_cases  # noqa: E402
from divrem_ref import divrem, inverse_series  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "divrem_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
SWITCHES = ("ZK_UPOLY_DIVREM_DIRECT_MAX", "ZK_UPOLY_DIVREM_LINEAR")
BAD, MISMATCH, UNSUP, PANIC_INVERSE = -20, -26, -25, -11


def _e(field, ints):
    return orc.from_ints(field, ints) if len(ints) else np.zeros((0, 4), dtype=np.uint64)


@pytest.fixture(scope="module")
def children():
    """{setting: ({(field id, case): (digest q, digest r)}, {(field id, shape): 'ok' | 'MISMATCH'})}: one child process per setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k not in SWITCHES}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"divrem {setting} ok" in r.stdout
        lines = [ln.split() for ln in r.stdout.splitlines()]
        out[setting] = ({(ln[1], ln[2]): (ln[3], ln[4]) for ln in lines if ln and ln[0] == "DIGEST"},
                        {(ln[1], ln[2]): ln[3] for ln in lines if ln and ln[0] == "EXACT"})
    return out


@pytest.fixture(scope="module")
def expected():
    """{(field id, case): (digest q, digest r)} from big-int schoolbook division, computed once"""
    out = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for name, a, b in small_cases(p, fi):
            q, r = divrem(a, b, p)
            out[(FIELD_IDS[fi], name)] = (digest(_e(field, q)), digest(_e(field, r)))
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_small_cases_match_schoolbook_on_every_path(children, expected, setting):
    """the direct kernel (DIRECT_MAX = 2048, LINEAR = 0), Newton (0, 0), the scan with Newton around it (0, 1) and the defaults give
    the bytes of big-int schoolbook division on every case and field"""
    got, _ = children[setting]
    assert len(expected) == 3 * (15 + 9) and set(got) == set(expected)
    for key, want in expected.items():
        print(setting, key, want, got[key])
        assert got[key] == want, (setting, key)


@pytest.mark.parametrize("setting", [s for s in SETTINGS if LARGE[s]])
def test_large_shapes_return_what_they_were_built_from(children, setting):
    """a = q0 b + r0 built with zk_upoly_mul / zk_upoly_add: divrem(a, b) == (q0, r0) on every coefficient (the result is unique)"""
    _, exact = children[setting]
    want = {(FIELD_IDS[fi], f"la{la}_lb{lb}") for la, lb, fields in LARGE[setting] for fi in fields}
    assert set(exact) == want
    for key in sorted(want):
        print(setting, key, exact[key])
        assert exact[key] == "ok", (setting, key)


@pytest.fixture(params=range(3), ids=FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def test_aliasing_skipped_results_empty_operands_and_stale_pool(fctx):
    fi, field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(41 + fi)
    ints = lambda h: orc.to_ints(field, h.coefficients())  # noqa: E731
    for la in (1, 6, 300, 3000):   # a == b: q = [1], r = la - 1 zeros; 3000 is past the direct kernel
        v = [rng.randrange(p) for _ in range(la - 1)] + [rng.randrange(1, p)]
        a = UP.new(ctx, _e(field, v))
        q, r = a.divmod(a)
        assert ints(q) == [1] and ints(r) == [0] * (la - 1)
        assert ints(a) == v   # the operand is not modified
    for la, lb in ((9, 4), (700, 300), (5000, 2), (5000, 3)):   # direct, direct, linear, Newton
        a, b = [rng.randrange(p) for _ in range(la)], [rng.randrange(p) for _ in range(lb - 1)] + [rng.randrange(1, p)]
        pa, pb = UP.new(ctx, _e(field, a)), UP.new(ctx, _e(field, b))
        want_q, want_r = divrem(a, b, p)
        assert ints(pa // pb) == want_q   # q only (r NULL)
        assert ints(pa % pb) == want_r    # r only (q NULL)
        q, r = divmod(pa, pb)
        assert (ints(q), ints(r)) == (want_q, want_r)
        assert ints(pa) == a and ints(pb) == b
        hq, hr = zk_amd.upoly_divrem_host(ctx, _e(field, a), _e(field, b))
        assert (orc.to_ints(field, hq), orc.to_ints(field, hr)) == (want_q, want_r)
    empty = UP.new(ctx, np.zeros((0, 4), dtype=np.uint64))
    b = UP.new(ctx, _e(field, [3, 0, 5]))
    q, r = empty.divmod(b)   # the empty dividend
    assert q.len() == 0 and r.len() == 0
    q, r = UP.new(ctx, _e(field, [7, 8])).divmod(b)   # la < lb: r a copy of a
    assert q.len() == 0 and ints(r) == [7, 8]
    q, r = UP.new(ctx, _e(field, [7, 8])).divmod(UP.new(ctx, _e(field, [0, 0, 0])))   # ... whatever b's top is: nothing is inverted
    assert q.len() == 0 and ints(r) == [7, 8]
    hq, hr = zk_amd.upoly_divrem_host(ctx, _e(field, [7, 8]), _e(field, [3, 0, 5]))
    assert hq.shape == (0, 4) and orc.to_ints(field, hr) == [7, 8]
    q, r = UP.new(ctx, _e(field, [6, 8, 10])).divmod(UP.new(ctx, _e(field, [2])))   # lb = 1: the empty remainder
    assert ints(q) == [3, 4, 5] and r.len() == 0
    # a large handle of non-zero values goes back to the pool; the next calls' blocks are cut from it or sit beside it
    big = UP.new(ctx, orc.fill_random(field, 5, 1 << 14))
    for n_vars in (9, 10, 13, 14):
        MLE.random(ctx, n_vars, 70 + n_vars).free()
    big.free()
    for la, lb in ((300, 7), (5000, 2), (5000, 40)):
        a, b = [rng.randrange(p) for _ in range(la)], [rng.randrange(p) for _ in range(lb - 1)] + [1]
        q, r = UP.new(ctx, _e(field, a)).divmod(UP.new(ctx, _e(field, b)))
        assert (ints(q), ints(r)) == divrem(a, b, p), (la, lb)


def test_inverse_series(fctx):
    """k = 0, 1, 2, 5, 256, 257, 2^12 + 1: f * (1 / f) = 1 mod z^k through zk_upoly_mul, and the big-int recurrence for k <= 257"""
    fi, field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(51 + fi)
    for k, lf in ((0, 3), (1, 4), (2, 1), (5, 9), (5, 3), (256, 256), (257, 40), (257, 300), ((1 << 12) + 1, (1 << 12) + 1), ((1 << 12) + 1, 17)):
        f = [rng.randrange(1, p)] + [rng.randrange(p) for _ in range(lf - 1)]
        pf = UP.new(ctx, _e(field, f))
        g = pf.inverse_series(k)
        assert g.len() == k
        if not k:
            continue
        back = orc.to_ints(field, (pf * g).coefficients())[:k]
        assert back == [1] + [0] * (k - 1), (k, lf)
        if k <= 257:
            want = inverse_series(f, k, p)
            assert orc.to_ints(field, g.coefficients()) == want, (k, lf)
            assert orc.to_ints(field, zk_amd.upoly_inverse_series_host(ctx, _e(field, f), k)) == want
    assert zk_amd.upoly_inverse_series_host(ctx, _e(field, [5]), 0).shape == (0, 4)


def _child_status(setting, la, lb):
    """a zero leading coefficient under one path's switches: the status and returned handles of eleven such calls, then of a good one"""
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import zk_amd; from zk_amd._lib import c, lib\n"
        "ctx = zk_amd.Context(zk_amd.BN254_FR, 0)\n"
        "a = zk_amd.UnivariatePolynomial.new(ctx, zk_amd.fe_from_ints(zk_amd.BN254_FR, list(range(1, %d + 1))))\n"
        "b = zk_amd.UnivariatePolynomial.new(ctx, zk_amd.fe_from_ints(zk_amd.BN254_FR, list(range(1, %d)) + [0]))\n"
        "g = zk_amd.UnivariatePolynomial.new(ctx, zk_amd.fe_from_ints(zk_amd.BN254_FR, list(range(1, %d + 1))))\n"
        "def call(d):\n"
        "    q, r = c.c_void_p(), c.c_void_p()\n"
        "    rc = lib.zk_upoly_divrem(ctx._h, a._h, d._h, c.byref(q), c.byref(r))\n"
        "    return rc, bool(q.value), bool(r.value)\n"
        "print('STATUS', [call(b) for _ in range(11)], call(g))\n" % (ROOT, la, lb, lb))
    env = dict({k: v for k, v in os.environ.items() if k not in SWITCHES}, **SETTINGS[setting])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return next(ln for ln in r.stdout.splitlines() if ln.startswith("STATUS"))


@pytest.mark.parametrize("setting,la,lb", [("direct", 300, 7), ("newton", 300, 7), ("linear", 5000, 2)])
def test_zero_leading_coefficient_on_each_path(setting, la, lb):
    """ZK_ERR_PANIC_INVERSE and no handle, eleven times over, and a good call on the same context afterwards.  (The blocks of a failed
    call go back to the context's pool through their scoped owners; the C ABI has no view of the pool to assert that through.)"""
    line = _child_status(setting, la, lb)
    print(line)
    fail = f"({PANIC_INVERSE}, False, False)"
    assert line == "STATUS [" + ", ".join([fail] * 11) + "] (0, True, True)", line


def test_error_table():
    field = zk_amd.BN254_FR
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    a = UP.new(ctx, orc.fill_random(field, 1, 8))
    b = UP.new(ctx, orc.fill_random(field, 2, 3))
    empty = UP.new(ctx, np.zeros((0, 4), dtype=np.uint64))
    b_other = UP.new(other, orc.fill_random(field, 2, 3))
    out = np.zeros((16, 4), dtype=np.uint64)
    ms = (c.c_double * 4)()
    q, r, h = c.c_void_p(), c.c_void_p(), c.c_void_p()
    u64p = c.POINTER(c.c_uint64)
    p = lambda v: v.ctypes.data_as(u64p)  # noqa: E731
    # nulls
    assert lib.zk_upoly_divrem(None, a._h, b._h, c.byref(q), c.byref(r)) == BAD
    assert lib.zk_upoly_divrem(ctx._h, None, b._h, c.byref(q), c.byref(r)) == BAD
    assert lib.zk_upoly_divrem(ctx._h, a._h, None, c.byref(q), c.byref(r)) == BAD
    assert lib.zk_upoly_divrem(ctx._h, a._h, b._h, None, None) == BAD
    assert lib.zk_upoly_divrem(ctx._h, a._h, empty._h, c.byref(q), c.byref(r)) == BAD   # lb = 0
    assert lib.zk_upoly_inverse_series(None, a._h, 4, c.byref(h)) == BAD
    assert lib.zk_upoly_inverse_series(ctx._h, None, 4, c.byref(h)) == BAD
    assert lib.zk_upoly_inverse_series(ctx._h, a._h, 4, None) == BAD
    assert lib.zk_upoly_divrem_host(None, p(out), 8, p(out), 3, p(out), p(out)) == BAD
    assert lib.zk_upoly_divrem_host(ctx._h, None, 8, p(out), 3, p(out), p(out)) == BAD
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), 8, None, 3, p(out), p(out)) == BAD
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), 8, p(out), 0, p(out), p(out)) == BAD
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), 8, p(out), 3, None, p(out)) == BAD
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), 8, p(out), 3, p(out), None) == BAD
    assert lib.zk_upoly_inverse_series_host(None, p(out), 3, 4, p(out)) == BAD
    assert lib.zk_upoly_inverse_series_host(ctx._h, None, 3, 4, p(out)) == BAD
    assert lib.zk_upoly_inverse_series_host(ctx._h, p(out), 3, 4, None) == BAD
    # another context's handle
    assert lib.zk_upoly_divrem(ctx._h, a._h, b_other._h, c.byref(q), c.byref(r)) == MISMATCH
    assert lib.zk_upoly_divrem(ctx._h, b_other._h, b._h, c.byref(q), c.byref(r)) == MISMATCH
    assert lib.zk_upoly_divrem(other._h, a._h, b._h, c.byref(q), c.byref(r)) == MISMATCH
    assert lib.zk_upoly_inverse_series(other._h, a._h, 4, c.byref(h)) == MISMATCH
    assert lib.zk_bench_upoly_divrem(other._h, a._h, b._h, 0, 1, ms) == MISMATCH
    assert not q.value and not r.value and not h.value
    # the zero that has to be inverted
    zero_lead = UP.new(ctx, orc.from_ints(field, [5, 6, 0]))
    assert lib.zk_upoly_divrem(ctx._h, a._h, zero_lead._h, c.byref(q), c.byref(r)) == PANIC_INVERSE
    assert lib.zk_upoly_divrem(ctx._h, a._h, zero_lead._h, c.byref(q), None) == PANIC_INVERSE
    zero_const = UP.new(ctx, orc.from_ints(field, [0, 6, 1]))
    assert lib.zk_upoly_inverse_series(ctx._h, zero_const._h, 5, c.byref(h)) == PANIC_INVERSE
    assert lib.zk_upoly_inverse_series(ctx._h, zero_const._h, 1, c.byref(h)) == PANIC_INVERSE
    assert lib.zk_upoly_inverse_series(ctx._h, empty._h, 5, c.byref(h)) == PANIC_INVERSE
    assert lib.zk_upoly_inverse_series_host(ctx._h, None, 0, 5, p(out)) == PANIC_INVERSE
    assert not q.value and not r.value and not h.value
    with pytest.raises(ZkError) as err:
        a.divmod(zero_lead)
    assert err.value.code == PANIC_INVERSE
    # the length rule, before the (short) buffers are read: BN254's two-adicity is 28; k = 2^28 needs 2^29-point transforms
    assert zk_amd.two_adicity(field) == 28
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), (1 << 28) + 2, p(out), 3, p(out), p(out)) == UNSUP
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), (1 << 28) + 2, p(out), 3, None, None) == UNSUP
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), (1 << 41), p(out), 2, p(out), p(out)) == UNSUP
    assert lib.zk_upoly_inverse_series_host(ctx._h, p(out), 3, (1 << 27) + 1, p(out)) == UNSUP
    assert lib.zk_upoly_inverse_series(ctx._h, a._h, 1 << 28, c.byref(h)) == UNSUP
    # k = 2^27 passes the rule; the call then stops at the missing out pointers, still before anything is read
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), (1 << 27) + 2, p(out), 3, None, p(out)) == BAD
    assert lib.zk_upoly_inverse_series_host(ctx._h, p(out), 3, 1 << 27, None) == BAD
    # empty results: nothing written, the pointer may be NULL
    out[:] = 7
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), 2, p(out), 3, None, p(out[8:])) == 0   # la < lb: q empty, r = a
    assert (out[8:10] == 7).all() and (out[10:] == 7).all()
    assert lib.zk_upoly_divrem_host(ctx._h, None, 0, p(out), 3, None, None) == 0
    assert lib.zk_upoly_divrem_host(ctx._h, p(out), 4, p(out), 1, p(out[8:]), None) == 0   # lb = 1: r empty
    assert lib.zk_upoly_inverse_series_host(ctx._h, p(out), 3, 0, None) == 0
    # the measurement hook
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 4, 1, ms) == BAD
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, -1, 1, ms) == BAD
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 0, 0, ms) == BAD
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 0, 1, None) == BAD
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, empty._h, 0, 1, ms) == BAD
    assert lib.zk_bench_upoly_divrem(ctx._h, b._h, a._h, 0, 1, ms) == BAD   # la < lb
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 2, 1, ms) == BAD   # the linear path wants lb = 2
    long_a = UP.new(ctx, orc.fill_random(field, 3, 3000))
    assert lib.zk_bench_upoly_divrem(ctx._h, long_a._h, b._h, 1, 1, ms) == BAD   # past the direct kernel's 2048
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 1, 1, ms) == 0 and ms[0] > 0 and ms[1] == 0
    assert lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, 3, 2, ms) == 0 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0 and ms[3] > 0
    two = UP.new(ctx, orc.fill_random(field, 4, 2))
    assert lib.zk_bench_upoly_divrem(ctx._h, long_a._h, two._h, 2, 1, ms) == 0 and ms[0] > 0
    assert lib.zk_bench_upoly_divrem(ctx._h, long_a._h, two._h, 0, 1, ms) == 0 and ms[0] > 0
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_upoly_divrem.cpp over zk.hpp: small cases by hand and one 2^12 constructed round trip"""
    exe = str(tmp_path / "test_upoly_divrem")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_upoly_divrem.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: upoly divrem host tests passed" in r.stdout
