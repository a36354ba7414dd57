"""Run by tests/test_gpu_upoly_evalmany.py in child processes (the library reads its ZK_* switches once per process), and imported by
it for the inputs, so that the parent and the children hold the same cases.

  evalmany  under ZK_UPOLY_EVALMANY_DIRECT_MAX (0: the transposed tree, 2^40: the direct kernel): a digest of
            zk_upoly_evaluate_many's values per case and field, after a run over stale pool blocks
  interp_xy under ZK_UPOLY_INTERP_XY_TREE_MIN (1: the weights from the tree path, 2^40: from the O(nx m) kernel): a digest of
            interpolate_xy's coefficients per case and field, and the status of the cases with a repeated x"""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

FIELD_IDS = ("bn254", "bls12_381", "bls12_377")
# n = L: 1, 2, 3; the bottom kernel alone and the first padded tree; the first NTT level; ping-pong parity of the levels; padding
SQUARE = (1, 2, 3, 127, 128, 129, 255, 256, 257, 512, 1024, 300, 1000)
LOPSIDED = ((0, 5), (1, 300), (5, 600), (257, 256), (1500, 40), (2048, 3))   # (L, n)
XY_SIZES = (2, 3, 129, 255, 256, 257, 1000)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def evalmany_cases(p, field_index):
    """[(name, coeffs, xs)] as canonical ints: seeded random values; the points hold 0, 1, p - 1 and repeats, the coefficients 0 and
    p - 1, wherever the case is long enough; one all-equal point vector and one all-zero polynomial"""
    rng = random.Random(0xE7A1 + field_index)
    out = []
    for L, n in [(s, s) for s in SQUARE] + list(LOPSIDED):
        assert L * n <= 1 << 21
        co = [rng.randrange(p) for _ in range(L)]
        xs = [rng.randrange(p) for _ in range(n)]
        for k, v in enumerate((0, 1, p - 1)):
            if n > k + 1:
                xs[k] = v
        if n >= 5:
            xs[n - 1] = xs[n // 2] = xs[3]
        if L >= 3:
            co[1], co[L - 1] = 0, p - 1
        out.append((f"L{L}_n{n}", co, xs))
    out.append(("all_equal_points", [rng.randrange(p) for _ in range(129)], [rng.randrange(p)] * 129))
    out.append(("zero_polynomial", [0] * 300, [rng.randrange(p) for _ in range(300)]))
    return out


def xy_cases(p, field_index):
    """[(name, xs, ys, repeated)]: distinct seeded xs holding 0, 1 and p - 1, ny = nx and ny < nx; then repeated xs at an index < m
    (repeated = True: the reference panics) and only among indices >= m"""
    rng = random.Random(0x1A9 + field_index)
    out = []
    for nx in XY_SIZES:
        xs = {0, 1, p - 1} if nx >= 3 else set()
        while len(xs) < nx:
            xs.add(rng.randrange(p))
        xs = sorted(xs)
        rng.shuffle(xs)
        for ny in (nx, nx - 1 if nx < 129 else nx // 2 + 1):
            out.append((f"nx{nx}_ny{ny}", xs, [rng.randrange(p) for _ in range(ny)], False))
    for name, xs, ny, bad in (("rep_small_bad", [1, 2, 1, 4], 4, True), ("rep_small_ok", [1, 2, 3, 5, 5], 3, False)):
        out.append((name, xs, [rng.randrange(p) for _ in range(ny)], bad))
    xs = rng.sample(range(1, 1 << 40), 300)
    bad, ok = list(xs), list(xs)
    bad[200] = bad[7]
    ok[260] = ok[250]
    out.append(("rep_300_bad", bad, [rng.randrange(p) for _ in range(300)], True))
    out.append(("rep_300_ok", ok, [rng.randrange(p) for _ in range(200)], False))
    return out


def _fields():
    import zk_amd

    return (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)


def check_evalmany():
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd import UnivariatePolynomial as UP

    for fi, field in enumerate(_fields()):
        ctx = zk_amd.Context(field, 0)
        p = orc.modulus(field)
        # stale pool data: freed random tables of the size classes the tree path draws its temporaries from
        for n_vars in (9, 10, 11):
            for s in range(6):
                MLE.random(ctx, n_vars, 900 + s + n_vars).free()
        rng = random.Random(77 + fi)
        co, xs = [rng.randrange(p) for _ in range(5)], [rng.randrange(p) for _ in range(300)]
        got = UP.new(ctx, orc.from_ints(field, co)).evaluate_many(UP.new(ctx, orc.from_ints(field, xs))).coefficients()
        print("DIGEST", FIELD_IDS[fi], "stale_L5_n300", digest(got))
        for name, co, xs in evalmany_cases(p, fi):
            pc = UP.new(ctx, orc.from_ints(field, co) if co else np.zeros((0, 4), dtype=np.uint64))
            got = pc.evaluate_many(UP.new(ctx, orc.from_ints(field, xs)))
            assert got.len() == len(xs)
            print("DIGEST", FIELD_IDS[fi], name, digest(got.coefficients()))
        ctx.close()
    print(f"evalmany ok (ZK_UPOLY_EVALMANY_DIRECT_MAX={os.environ.get('ZK_UPOLY_EVALMANY_DIRECT_MAX')})")


def check_interp_xy():
    import zk_amd
    from oracle import binding as orc
    from zk_amd import UnivariatePolynomial as UP
    from zk_amd import ZkError

    for fi, field in enumerate(_fields()):
        ctx = zk_amd.Context(field, 0)
        p = orc.modulus(field)
        for name, xs, ys, _ in xy_cases(p, fi):
            try:
                got = UP.interpolate_xy(ctx, orc.from_ints(field, xs), orc.from_ints(field, ys))
                assert got.len() == len(xs)
                print("DIGEST", FIELD_IDS[fi], name, digest(got.coefficients()))
            except ZkError as e:
                print("DIGEST", FIELD_IDS[fi], name, f"error{e.code}")
        ctx.close()
    print(f"interp_xy ok (ZK_UPOLY_INTERP_XY_TREE_MIN={os.environ.get('ZK_UPOLY_INTERP_XY_TREE_MIN')})")


if __name__ == "__main__":
    {"evalmany": check_evalmany, "interp_xy": check_interp_xy}[sys.argv[1]]()
