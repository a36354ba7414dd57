"""Run by tests/test_gpu_upoly_divrem.py in child processes (the library reads its ZK_* switches once per process), and imported by it
for the inputs, so that the parent and the children hold the same cases.

  python divrem_check.py <setting>    setting: direct | newton | linear | model
      under ZK_UPOLY_DIVREM_DIRECT_MAX / ZK_UPOLY_DIVREM_LINEAR as the parent sets them: a digest of zk_upoly_divrem's q and r per
      small case and field (after a run over stale pool blocks), and the setting's large shapes by exact construction: q0, r0 and b
      drawn, a = q0 b + r0 formed with zk_upoly_mul / zk_upoly_add, divrem(a, b) required to return (q0, r0) on every coefficient"""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402  (the structured worst-case limbs, shared with the GKR wiring tests)

FIELD_IDS = ("bn254", "bls12_381", "bls12_377")
# (la, lb): k = 1, lb = 1, la < lb, and k and lb - 1 on both sides of 2^8, where the product switches from the direct kernel to the NTT
SHAPES = ((1, 1), (5, 1), (5, 5), (5, 6), (7, 3), (64, 64), (65, 2), (300, 2), (300, 129), (257, 128), (511, 256), (513, 255), (2048, 2),
          (2048, 1025), (2047, 257))
# exact-construction shapes per setting: (la, lb, fields)
LARGE = {
    "direct": (),
    "newton": (((1 << 12) + 1, 3, (0, 1, 2)), ((1 << 14) + 5, (1 << 13) - 3, (0, 1, 2)), (1 << 13, (1 << 13) - 1, (0, 1, 2))),
    # the last: 258 chunks of 4096 on k_divlin_carry's 256 threads, two per thread (threads 129.. idle), a top chunk of one coefficient
    "linear": (((1 << 16) + 1, 2, (0, 1, 2)), ((1 << 18) + 3, 2, (0, 1, 2)), ((1 << 20) + 4097, 2, (0,))),
    "model": (((1 << 18) + 1, (1 << 17) - 1, (0, 1, 2)), (1 << 20, 2, (0,))),
}
SETTINGS = {
    "direct": dict(ZK_UPOLY_DIVREM_DIRECT_MAX="2048", ZK_UPOLY_DIVREM_LINEAR="0"),
    "newton": dict(ZK_UPOLY_DIVREM_DIRECT_MAX="0", ZK_UPOLY_DIVREM_LINEAR="0"),
    "linear": dict(ZK_UPOLY_DIVREM_DIRECT_MAX="0", ZK_UPOLY_DIVREM_LINEAR="1"),
    "model": dict(),
}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def small_cases(p, field_index):
    """[(name, a, b)] as canonical ints; every b[-1] is non-zero"""
    rng = random.Random(0xD17 + field_index)
    rv = lambda n: [rng.randrange(p) for _ in range(n)]  # noqa: E731
    out = []
    for la, lb in SHAPES:
        b = rv(lb)
        b[-1] = rng.randrange(1, p)
        out.append((f"la{la}_lb{lb}", rv(la), b))
    a = rv(40)
    a[-3:] = [0, 0, 0]
    out.append(("zero_topped_dividend", a, rv(6) + [rng.randrange(1, p)]))
    out.append(("divisor_b0_zero", rv(33), [0] + rv(3) + [rng.randrange(1, p)]))
    out.append(("divisor_b0_zero_long", rv(600), [0] + rv(298) + [rng.randrange(1, p)]))
    a = rv(300)
    out.append(("linear_z_one", a, [p - 1, 1]))
    out.append(("linear_z_zero", a, [0, 1]))
    out.append(("linear_c0_c1", a, [rng.randrange(1, p), rng.randrange(2, p)]))
    out.append(("linear_c0_c1_5000", rv(5000), [rng.randrange(1, p), rng.randrange(2, p)]))   # a second, ragged chunk of the scan
    w = worst_case_values(p, field_index, 237)
    out.append(("worst_case_limbs", w[:200], w[200:236] + [w[236] or 1]))
    out.append(("worst_case_limbs_linear", w[:200], [w[201] or 1, w[202] or 1]))
    return out


def _fields():
    import zk_amd

    return (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)


def check(setting):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd import UnivariatePolynomial as UP

    for name, value in SETTINGS[setting].items():
        assert os.environ.get(name) == value, (name, os.environ.get(name))
    for fi, field in enumerate(_fields()):
        ctx = zk_amd.Context(field, 0)
        p = orc.modulus(field)
        e = lambda ints: orc.from_ints(field, ints) if len(ints) else np.zeros((0, 4), dtype=np.uint64)  # noqa: E731
        # stale pool data: freed random tables of the size classes the paths draw their results and temporaries from
        for n_vars in (1, 5, 8, 9, 10, 11, 12):
            for s in range(4):
                MLE.random(ctx, n_vars, 900 + s + n_vars).free()
        for name, a, b in small_cases(p, fi):
            q, r = UP.new(ctx, e(a)).divmod(UP.new(ctx, e(b)))
            print("DIGEST", FIELD_IDS[fi], name, digest(q.coefficients()), digest(r.coefficients()))
        for la, lb, fields in LARGE[setting]:
            if fi not in fields:
                continue
            k = la - lb + 1
            q0, b = orc.fill_random(field, 7000 + la % 1000 + fi, k), orc.fill_random(field, 7100 + lb % 1000 + fi, lb)
            b[lb - 1] = orc.from_int(field, 0x1234567 + fi)   # a non-zero leading coefficient
            pq, pb = UP.new(ctx, q0), UP.new(ctx, b)
            a = pq * pb
            if lb > 1:
                r0 = orc.fill_random(field, 7200 + fi, lb - 1)
                a = a + UP.new(ctx, r0)
            else:
                r0 = np.zeros((0, 4), dtype=np.uint64)
            assert a.len() == la
            q, r = a.divmod(pb)
            ok = q.len() == k and r.len() == lb - 1 and np.array_equal(q.coefficients(), q0) and np.array_equal(r.coefficients(), r0)
            print("EXACT", FIELD_IDS[fi], f"la{la}_lb{lb}", "ok" if ok else "MISMATCH")
        ctx.close()
    print(f"divrem {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
