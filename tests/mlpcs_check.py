"""Run by tests/test_gpu_mlpcs.py in child processes (the library reads its ZK_* switches once per process), and imported by it for the
settings, so that the parent and the children hold the same cases.

  python mlpcs_check.py <setting>    setting: default | fused | tables
      under ZK_MLPCS_ROUND as the parent sets it (1 = the fused round kernel, 0 = the eq table with the two-table round sums): a digest of
      root, value and proof of every opening of tests/mlpcs_ref.py's GPU cases (each proof is given to zk_mlpcs_verify_host, the source
      table is freed after the commitment) and, in the default child, of every zk_mle_eq_sums of its cases (the table is checked to be
      left intact) and of the BN254 ones that the parent checks against the C oracle"""
import hashlib
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fri_ref  # noqa: E402
import mlpcs_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

SWITCH = "ZK_MLPCS_ROUND"
SETTINGS = {"default": {}, "fused": {SWITCH: "1"}, "tables": {SWITCH: "0"}}
BIG_SEED = 0xB16E9


def digest(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def case_key(case):
    return "n%d_b%d_f%d_q%d" % case


def big_tail(p, n):
    """the tail of an oracle-checked case of n variables: seeded random entries (every Hi entry non-zero) and one p - 1"""
    rng = random.Random(BIG_SEED + n)
    tail = [rng.randrange(2, p - 1) for _ in range(n - 1)]
    tail[3] = p - 1
    return tail


def check(setting):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE

    assert os.environ.get(SWITCH) == SETTINGS[setting].get(SWITCH), os.environ.get(SWITCH)
    fields = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)
    ctxs = [zk_amd.Context(field, 0) for field in fields]
    for fi, field in enumerate(fields):
        ctx, p = ctxs[fi], orc.modulus(field)
        for n_vars in (0, 1, 4, 8, 10, 12, 14, 16):   # stale pool data in the size classes of the tables
            MLE.random(ctx, n_vars, 900 + n_vars).free()
        if setting != "default":
            continue
        for n in ref.EQ_SUMS_VARS:
            table, tail = ref.eq_sums_case(fi, n, worst_case_values)
            src = orc.from_ints(field, table)
            t = MLE.new(ctx, n, src)
            got = zk_amd.eq_sums(t, orc.from_ints(field, tail) if tail else [])
            assert np.array_equal(t.evaluation_slice(), src), (fi, n, "the table changed")
            print("SUMS", fri_ref.FIELD_IDS[fi], "n%d" % n, digest(got.tobytes()))
            t.free()
    if setting == "default":   # BN254: the longer runs and the smallest table whose launch takes a second trip; expected: the oracle's (the parent)
        for n in ref.ORACLE_SUMS_VARS:
            t = MLE.random(ctxs[0], n, BIG_SEED + n)
            got = zk_amd.eq_sums(t, orc.from_ints(0, big_tail(orc.modulus(0), n)))
            print("BIGSUMS", fri_ref.FIELD_IDS[0], "n%d" % n, digest(got.tobytes()))
            t.free()
    for case in ref.GPU_CASES:
        n, b, f, q = case
        fi = ref.case_field(case)
        table, shift, seed, z = ref.case_inputs(fi, case, worst_case_values)
        t = MLE.new(ctxs[fi], n, orc.from_ints(fi, table))
        com = zk_amd.MultilinearCommitment.commit(t, b, orc.from_int(fi, shift))
        t.free()   # the commitment owns what it needs
        root = com.root()
        value, proof = com.open(orc.from_ints(fi, z), f, q, seed)
        assert zk_amd.mlpcs_verify(fi, root, orc.from_ints(fi, z), value, proof, b, f, q, orc.from_int(fi, shift), seed), case
        print("PROOF", fri_ref.FIELD_IDS[fi], case_key(case), digest(root + value.tobytes() + proof))
        com.free()
    for ctx in ctxs:
        ctx.close()
    print(f"mlpcs {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
