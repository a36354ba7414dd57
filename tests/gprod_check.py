"""Run by tests/test_gpu_gprod.py in child processes (the library reads its ZK_* switches once per process), and imported by it for the
settings, so that the parent and the children hold the same cases.

  python gprod_check.py <setting>    setting: default | fuse1 | fuse2 | fuse3
      under ZK_GPROD_TREE_FUSE as the parent sets it (the levels of the product tree per launch above the LDS stage): a digest of product,
      proof, point and claim of every proof of tests/gprod_ref.py's GPU cases (each proof is given to zk_gprod_verify_host, the table is
      checked to be left intact), of every zk_mle_product_tree of its sizes on the three fields with a NULL shift and with p - 1, and of
      the BN254 trees that the parent checks against the C oracle: 2^20 elements on every setting and, with one level per launch, the
      smallest table at which the capped grid takes a second trip"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gprod_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

SWITCH = "ZK_GPROD_TREE_FUSE"
SETTINGS = {"default": {}, "fuse1": {SWITCH: "1"}, "fuse2": {SWITCH: "2"}, "fuse3": {SWITCH: "3"}}
FIELD_IDS = ("bn254", "bls12_381", "bls12_377")
BIG_SEED = 0x69D0D
BIG_VARS = 20


def digest(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def case_key(case):
    return "n%d_v%d_%s" % (case[0], case[1], case[2] or "plain")


def big_vars(setting):
    """the sizes of the oracle-checked trees of a setting"""
    fuse = int(SETTINGS[setting].get(SWITCH, ref.FUSE_DEFAULT))
    return (BIG_VARS,) + ((ref.SECOND_TRIP_VARS[fuse],) if ref.SECOND_TRIP_VARS[fuse] < 25 else ())


def tree_case(field_index, n, p):
    """the table of one zk_mle_product_tree case: worst-case limb patterns mixed with seeded values, no zero and no 1 (so no entry
    vanishes under either shift)"""
    import random
    rng = random.Random(0x7EE + 1000 * field_index + n)
    worst = [x % p for x in worst_case_values(p, field_index, 256) if x % p > 1]
    return [rng.choice(worst) if rng.random() < 0.3 else rng.randrange(2, p) for _ in range(1 << n)]


def oracle_heap(orc, field, table):
    """zk_mle_product_tree's heap by the C oracle's arithmetic: repeated products of the halves"""
    n = table.shape[0].bit_length() - 1
    heap = np.zeros((1 << n, 4), dtype=np.uint64)
    heap[0] = orc.from_int(field, 1)
    cur = table
    for j in range(n - 1, -1, -1):
        cur = orc.prod_reduce(field, j, [cur[:1 << j], cur[1 << j:]])
        heap[1 << j:2 << j] = cur
    return heap


def check(setting):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE

    assert os.environ.get(SWITCH) == SETTINGS[setting].get(SWITCH), os.environ.get(SWITCH)
    fields = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)
    ctxs = [zk_amd.Context(field, 0) for field in fields]
    for fi, field in enumerate(fields):
        ctx, p = ctxs[fi], orc.modulus(field)
        for n_vars in (0, 1, 4, 8, 10, 12, 14):   # stale pool data in the size classes of the tables
            MLE.random(ctx, n_vars, 900 + n_vars).free()
        for n in ref.TREE_VARS:
            src = orc.from_ints(field, tree_case(fi, n, p))
            t = MLE.new(ctx, n, src)
            for name, shift in (("null", None), ("minus_one", orc.from_int(field, p - 1))):
                heap = zk_amd.product_tree(t, shift)
                print("TREE", FIELD_IDS[fi], "n%d_%s" % (n, name), digest(heap.evaluation_slice().tobytes()))
                heap.free()
            assert np.array_equal(t.evaluation_slice(), src), (fi, n, "the table changed")
            t.free()
    for n in big_vars(setting):   # BN254, the oracle's generator's table; expected: the oracle's (the parent)
        t = MLE.random(ctxs[0], n, BIG_SEED + n)
        heap = zk_amd.product_tree(t)
        print("BIGTREE", FIELD_IDS[0], "n%d" % n, digest(heap.evaluation_slice().tobytes()))
        heap.free()
        t.free()
    for case in ref.GPU_CASES:
        fi, table, shift, seed = ref.case_inputs(case, worst_case_values)
        src = orc.from_ints(fi, table)
        t = MLE.new(ctxs[fi], case[0], src)
        sv = None if shift is None else orc.from_int(fi, shift)
        product, proof, point, claim = zk_amd.grand_product_prove(t, seed, sv)
        assert np.array_equal(t.evaluation_slice(), src), (case, "the table changed")
        got = zk_amd.grand_product_verify(fi, case[0], seed, product, proof, sv)
        assert got is not None and np.array_equal(got[0], point) and np.array_equal(got[1], claim), case
        assert zk_amd.grand_product_verify_table(t, seed, product, proof, sv), case
        print("PROOF", FIELD_IDS[fi], case_key(case), digest(product.tobytes() + proof + point.tobytes() + claim.tobytes()))
        t.free()
    for ctx in ctxs:
        ctx.close()
    print(f"gprod {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
