"""zk_upoly_evaluate_many on the device (UnivariatePolynomial::evaluate, univariate_poly.rs:29-40, at a vector of points): both
paths bit for bit against Python Horner in child processes, p == xs / n = 0 / stale pool blocks, a mid size against
zk_upoly_evaluate, the 2^18 round trip through interpolate_xy, interpolate_xy's weights from either path (ZK_UPOLY_INTERP_XY_TREE_MIN),
the error table and the C++ mirror."""
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
from evalmany_check import FIELD_IDS, digest, evalmany_cases, xy_cases  # noqa: E402
from evalmany_ref import horner_many  # noqa: E402
from interp_ref import lagrange  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "evalmany_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
SWITCHES = ("ZK_UPOLY_EVALMANY_DIRECT_MAX", "ZK_UPOLY_INTERP_XY_TREE_MIN")
BAD, MISMATCH, UNSUP, PANIC_INVERSE = -20, -26, -25, -11


def _children(mode, settings):
    """{setting name: {(field id, case): digest}}: one child process per setting of the switch, all fields in it"""
    out = {}
    for name, extra in settings.items():
        env = dict({k: v for k, v in os.environ.items() if k not in SWITCHES}, **extra)
        r = subprocess.run([sys.executable, CHECK, mode], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{mode} {extra} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"{mode} ok" in r.stdout
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("DIGEST")]
        out[name] = {(f, case): d for _, f, case, d in lines}
    return out


@pytest.fixture(scope="module")
def evalmany_children():
    return _children("evalmany", {"tree": dict(ZK_UPOLY_EVALMANY_DIRECT_MAX="0"), "direct": dict(ZK_UPOLY_EVALMANY_DIRECT_MAX=str(1 << 40))})


@pytest.fixture(scope="module")
def xy_children():
    return _children("interp_xy", {"tree": dict(ZK_UPOLY_INTERP_XY_TREE_MIN="1"), "kernel": dict(ZK_UPOLY_INTERP_XY_TREE_MIN=str(1 << 40))})


@pytest.fixture(params=range(3), ids=FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def _e(field, ints):
    return orc.from_ints(field, ints) if len(ints) else np.zeros((0, 4), dtype=np.uint64)


@pytest.mark.parametrize("fi", range(3), ids=FIELD_IDS)
def test_every_shape_on_both_paths_matches_horner(evalmany_children, fi):
    """the tree path (switch 0) and the direct path (switch 2^40) give the same bytes as Python Horner on every case"""
    field = FIELDS[fi]
    p = orc.modulus(field)
    tree, direct = evalmany_children["tree"], evalmany_children["direct"]
    cases = evalmany_cases(p, fi)
    assert len(cases) == 13 + 6 + 2
    rng = random.Random(77 + fi)   # the children's stale-pool case
    cases.append(("stale_L5_n300", [rng.randrange(p) for _ in range(5)], [rng.randrange(p) for _ in range(300)]))
    for name, co, xs in cases:
        want = digest(_e(field, horner_many(co, xs, p)))
        key = (FIELD_IDS[fi], name)
        print(name, want, tree[key], direct[key])
        assert tree[key] == want, ("tree", name)
        assert direct[key] == want, ("direct", name)
    assert len([k for k in tree if k[0] == FIELD_IDS[fi]]) == len(cases) == len([k for k in direct if k[0] == FIELD_IDS[fi]])


def test_aliased_operands_empty_points_and_stale_pool(fctx):
    fi, field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(31 + fi)
    for n in (1, 6, 300):   # p == xs
        v = [rng.randrange(p) for _ in range(n)]
        q = UP.new(ctx, _e(field, v))
        got = q.evaluate_many(q)
        assert orc.to_ints(field, got.coefficients()) == horner_many(v, v, p)
        assert orc.to_ints(field, q.coefficients()) == v   # the operand is not modified
    q = UP.new(ctx, _e(field, [1, 2, 3]))
    empty = UP.new(ctx, np.zeros((0, 4), dtype=np.uint64))
    assert q.evaluate_many(empty).len() == 0
    assert orc.to_ints(field, empty.evaluate_many(q).coefficients()) == [0, 0, 0]
    assert orc.to_ints(field, q.evaluate_many([0, 1, 2, p - 1, p + 2]).coefficients()) == [1, 6, 17, 2, 17]   # Python ints, mod p
    assert zk_amd.upoly_evaluate_many_host(ctx, _e(field, [1, 2, 3]), _e(field, [])).shape == (0, 4)
    # a large handle of non-zero values goes back to the pool; the next calls' blocks are cut from it or sit beside it
    big = UP.new(ctx, orc.fill_random(field, 5, 1 << 14))
    for n_vars in (9, 10, 14):
        MLE.random(ctx, n_vars, 70 + n_vars).free()
    big.free()
    co, xs = [rng.randrange(p) for _ in range(5)], [rng.randrange(p) for _ in range(300)]
    want = horner_many(co, xs, p)
    assert orc.to_ints(field, UP.new(ctx, _e(field, co)).evaluate_many(UP.new(ctx, _e(field, xs))).coefficients()) == want
    assert orc.to_ints(field, zk_amd.upoly_evaluate_many_host(ctx, _e(field, co), _e(field, xs))) == want


def test_mid_size_with_the_default_model_matches_evaluate(fctx):
    """n = 2^16 + 1, L = 2^16 - 1 on whatever the cost model picks: 64 seeded positions against zk_upoly_evaluate at the same points"""
    fi, field, ctx = fctx
    n, L = (1 << 16) + 1, (1 << 16) - 1
    xs = orc.fill_random(field, 810 + fi, n)
    q = UP.new(ctx, orc.fill_random(field, 820 + fi, L))
    got = q.evaluate_many(UP.new(ctx, xs))
    assert got.len() == n
    vals = got.coefficients()
    for i in random.Random(n + fi).sample(range(n), 64):
        assert np.array_equal(q.evaluate(xs[i]), vals[i]), i


def test_round_trip_through_interpolate_xy_at_2p18():
    """evaluate_many(interpolate_xy(xs, ys), xs) == ys on all 2^18 values, xs = i g + 7 (distinct by construction: g != 0, i < p)"""
    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    p = orc.modulus(field)
    n, g = 1 << 18, 0x1234567890ABCDEF1234567890ABCDEF
    xs = UP.new(ctx, orc.from_ints(field, [(i * g + 7) % p for i in range(n)]))
    ys = orc.fill_random(field, 4242, n)
    back = UP.interpolate_xy(ctx, xs, UP.new(ctx, ys)).evaluate_many(xs)
    assert back.len() == n
    assert np.array_equal(back.coefficients(), ys)
    ctx.close()


@pytest.mark.parametrize("fi", range(3), ids=FIELD_IDS)
def test_interpolate_xy_weights_from_either_path(xy_children, fi):
    """ZK_UPOLY_INTERP_XY_TREE_MIN = 1 (d_i = M'(x_i) by the tree path) and 2^40 (k_interp_denoms): byte-identical coefficients,
    equal to the Lagrange restatement up to 300 points; a repeated x at an index < m is ZK_ERR_PANIC_INVERSE under both, one only
    among indices >= m no error under both"""
    field = FIELDS[fi]
    p = orc.modulus(field)
    tree, kern = xy_children["tree"], xy_children["kernel"]
    cases = xy_cases(p, fi)
    assert len(cases) == 2 * 7 + 4
    for name, xs, ys, repeated in cases:
        key = (FIELD_IDS[fi], name)
        print(name, tree[key], kern[key])
        assert tree[key] == kern[key], name
        if repeated:
            assert tree[key] == f"error{PANIC_INVERSE}", name
        else:
            assert not tree[key].startswith("error"), name
            if len(xs) <= 300:
                assert tree[key] == digest(_e(field, lagrange(xs, ys, p))), name


def test_error_table():
    field = zk_amd.BN254_FR
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    a = UP.new(ctx, orc.fill_random(field, 1, 8))
    b_other = UP.new(other, orc.fill_random(field, 2, 8))
    out = np.zeros((16, 4), dtype=np.uint64)
    ms = (c.c_double * 6)()
    h = c.c_void_p()
    u64p = c.POINTER(c.c_uint64)
    p = lambda v: v.ctypes.data_as(u64p)  # noqa: E731
    assert lib.zk_upoly_evaluate_many(None, a._h, a._h, c.byref(h)) == BAD
    assert lib.zk_upoly_evaluate_many(ctx._h, None, a._h, c.byref(h)) == BAD
    assert lib.zk_upoly_evaluate_many(ctx._h, a._h, None, c.byref(h)) == BAD
    assert lib.zk_upoly_evaluate_many(ctx._h, a._h, a._h, None) == BAD
    assert lib.zk_upoly_evaluate_many_host(None, p(out), 3, p(out), 3, p(out)) == BAD
    assert lib.zk_upoly_evaluate_many_host(ctx._h, None, 3, p(out), 3, p(out)) == BAD
    assert lib.zk_upoly_evaluate_many_host(ctx._h, p(out), 3, None, 3, p(out)) == BAD
    assert lib.zk_upoly_evaluate_many_host(ctx._h, p(out), 3, p(out), 3, None) == BAD
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, a._h, a._h, 3, 1, ms) == BAD
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, a._h, a._h, 0, 0, ms) == BAD
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, a._h, a._h, 0, 1, None) == BAD
    assert lib.zk_upoly_evaluate_many(ctx._h, a._h, b_other._h, c.byref(h)) == MISMATCH
    assert lib.zk_upoly_evaluate_many(ctx._h, b_other._h, a._h, c.byref(h)) == MISMATCH
    assert lib.zk_upoly_evaluate_many(other._h, a._h, a._h, c.byref(h)) == MISMATCH
    assert lib.zk_bench_upoly_evaluate_many(other._h, a._h, a._h, 0, 1, ms) == MISMATCH
    assert not h.value
    # the length rule, checked before the (short) buffers are read: BN254's two-adicity is 28, so N = 2^28 has no tree path (its
    # largest transform is 2N points) and n L = 2^56 products are past the direct path's 2^40
    assert zk_amd.two_adicity(field) == 28
    assert lib.zk_upoly_evaluate_many_host(ctx._h, p(out), 1 << 28, p(out), 1 << 28, p(out)) == UNSUP
    assert lib.zk_upoly_evaluate_many_host(ctx._h, p(out), 1 << 28, p(out), 1 << 28, None) == UNSUP
    # L = 2^28, n = 1: 2^28 products, the direct path may run, so the rule passes; the call then stops at the missing out, still
    # before anything is read
    assert lib.zk_upoly_evaluate_many_host(ctx._h, p(out), 1 << 28, p(out), 1, None) == BAD
    # empty results: nothing written, out may be NULL
    assert lib.zk_upoly_evaluate_many_host(ctx._h, p(out), 3, p(out), 0, None) == 0
    assert lib.zk_upoly_evaluate_many_host(ctx._h, None, 0, None, 0, None) == 0
    # the empty polynomial: n zeros
    out[:] = 7
    assert lib.zk_upoly_evaluate_many_host(ctx._h, None, 0, p(out), 5, p(out)) == 0
    assert not out[:5].any() and (out[5:] == 7).all()
    # the measurement hook refuses the tree path where the rule does not offer it, and runs where it does
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, a._h, a._h, 2, 1, ms) == 0 and ms[0] > 0
    assert lib.zk_bench_upoly_evaluate_many(ctx._h, a._h, a._h, 1, 1, ms) == 0 and ms[0] > 0 and ms[1] == 0
    for q in (a, b_other):
        q.free()
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_upoly_evalmany.cpp over zk.hpp: small cases by hand and one 2^12 round trip"""
    exe = str(tmp_path / "test_upoly_evalmany")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_upoly_evalmany.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: upoly evaluate_many host tests passed" in r.stdout
