"""Run by tests/test_gpu_zerocheck.py in a child process, and imported by it for the case keys, so that parent and child hold the same
cases.

  python zerocheck_check.py
      a digest of proof, point and claims of every proof of tests/zerocheck_ref.py's cases (each is given to zk_zerocheck_verify_host,
      whose verdict is printed with it, and the tables are checked to be left intact); a digest of zk_mle_gate_sums of every case's
      tables against a seeded tail; and for the gate x0 at every n = 1 .. 13 zk_mle_gate_sums against zk_mle_eq_sums of the same table
      and tail, bit for bit"""
import hashlib
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zerocheck_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

FIELD_IDS = ("bn254", "bls12_381", "bls12_377")
X0_VARS = tuple(range(1, 14))


def digest(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def case_tail(case, p):
    """the n - 1 elements zk_mle_gate_sums of a case runs against"""
    rng = random.Random(0x7A1 + ref.hash_case(case))
    return [rng.randrange(p) for _ in range(case[0] - 1)]


def x0_table(fi, n, p):
    rng = random.Random(0x0E0 + 100 * fi + n)
    worst = [x % p for x in worst_case_values(p, fi, 256)]
    return [rng.choice(worst) if rng.random() < 0.3 else rng.randrange(p) for _ in range(1 << n)]


def check():
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE

    fields = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)
    ctxs = [zk_amd.Context(field, 0) for field in fields]
    for ctx in ctxs:
        for n_vars in (0, 1, 4, 8, 10, 12):   # stale pool data in the size classes of the scratch
            MLE.random(ctx, n_vars, 700 + n_vars).free()
    for case in ref.CASES:
        fi, gate, tables, seed = ref.case_inputs(case, worst_case_values)
        p = orc.modulus(fi)
        g = zk_amd.Gate(fi, gate[0], gate[1])
        srcs = [orc.from_ints(fi, t) for t in tables]
        tabs = [MLE.new(ctxs[fi], case[0], s) for s in srcs]
        proof, point, claims = zk_amd.zerocheck_prove(tabs, g, seed)
        got = zk_amd.zerocheck_verify(g, case[0], seed, proof)
        assert got is None or (np.array_equal(got[0], point) and np.array_equal(got[1], claims)), case
        print("PROOF", FIELD_IDS[fi], ref.case_key(case), digest(proof + point.tobytes() + claims.tobytes()), int(got is not None))
        tail = orc.from_ints(fi, case_tail(case, p)) if case[0] > 1 else None
        print("SUMS", FIELD_IDS[fi], ref.case_key(case), digest(zk_amd.gate_sums(tabs, g, tail).tobytes()), 0)
        for t, s in zip(tabs, srcs):
            assert np.array_equal(t.evaluation_slice(), s), (case, "a table changed")
            t.free()
    for fi, field in enumerate(fields):
        p = orc.modulus(field)
        g = zk_amd.Gate(field, 1, ref.GATES["x0"][1])
        for n in X0_VARS:
            t = MLE.new(ctxs[fi], n, orc.from_ints(field, x0_table(fi, n, p)))
            rng = random.Random(0x0E1 + n)
            tail = orc.from_ints(field, [rng.randrange(p) for _ in range(n - 1)]) if n > 1 else None
            ours = zk_amd.gate_sums([t], g, tail)
            theirs = zk_amd.eq_sums(t, tail if n > 1 else np.zeros((0, 4), dtype=np.uint64))
            assert ours.shape == (2, 4) and np.array_equal(ours, np.asarray(theirs).reshape(2, 4)), (fi, n)
            print("X0", FIELD_IDS[fi], "n%d" % n, digest(ours.tobytes()), 0)
            t.free()
    for ctx in ctxs:
        ctx.close()
    print("zerocheck ok")


if __name__ == "__main__":
    check()
