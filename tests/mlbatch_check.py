"""Run by tests/test_gpu_mlbatch.py in child processes (the library reads its ZK_* switches once per process), and imported by it for the
settings, so that the parent and the children hold the same cases.

  python mlbatch_check.py <setting>    setting: default | unfused | fused
      under ZK_MLBATCH_FUSE_FOLD as the parent sets it (1 = the combine-and-fold kernel, 0 = the linear combination into a scratch layer
      and FRI's fold): a digest of root, values and proof of every opening of tests/mlbatch_ref.py's GPU cases (each proof is given to
      zk_mlbatch_verify_host, the source tables are freed after the commitment) and, in the default child, of every zk_mle_eq_sums_many
      and zk_mle_lincomb case (the sources are checked to be left intact), the BN254 sums that the parent checks against the C oracle, and
      the sampled outputs of the lincomb whose grid-stride loop takes a second trip"""
import hashlib
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fri_ref  # noqa: E402
import mlbatch_ref as ref  # noqa: E402
import mlpcs_ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

SWITCH = "ZK_MLBATCH_FUSE_FOLD"
SETTINGS = {"default": {}, "unfused": {SWITCH: "0"}, "fused": {SWITCH: "1"}}
BIG_SEED = 0xBA7C4
ORACLE_SUMS_VARS = (21, mlpcs_ref.SECOND_TRIP_VARS)   # BN254, 2 points: runs of 2^9 elements; the capped grid's second trip
SUMS_POINTS = (1, ref.POINTS_PER_PASS, ref.POINTS_PER_PASS + 1)
BIG_LINCOMB_K, BIG_LINCOMB_SAMPLES = 3, 4096


def digest(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def case_key(case):
    return "n%d_b%d_f%d_q%d_k%d_m%d" % case


def big_tails(p, n, count=2):
    """the tails of an oracle-checked case of n variables: seeded random entries (every Hi entry non-zero) and one p - 1 each"""
    rng = random.Random(BIG_SEED + n)
    tails = [[rng.randrange(2, p - 1) for _ in range(n - 1)] for _ in range(count)]
    for j, tail in enumerate(tails):
        tail[3 + j] = p - 1
    return tails


def big_lincomb(p):
    """(n, seeds of the k tables, coefficients, sampled indices) of the lincomb that takes a second trip: the first and last 64 elements,
    both sides of the trip boundary, seeded ones for the rest"""
    n = ref.LINCOMB_SECOND_TRIP_VARS
    rng = random.Random(BIG_SEED + 7)
    coeffs = [rng.randrange(p), p - 1, rng.randrange(p)]
    size, trip = 1 << n, ref.LINCOMB_MAX_BLOCKS * mlpcs_ref.THREADS * ref.LINCOMB_ELEMS_PER_THREAD
    idx = set(range(64)) | set(range(size - 64, size)) | set(range(trip - 2, trip + 2))
    while len(idx) < BIG_LINCOMB_SAMPLES + 128:
        idx.add(rng.randrange(size))
    return n, [BIG_SEED + 100 + c for c in range(BIG_LINCOMB_K)], coeffs, sorted(idx)


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
        for n in mlpcs_ref.EQ_SUMS_VARS:
            for np_ in SUMS_POINTS:
                table, tails = ref.eq_sums_many_case(fi, n, np_, worst_case_values)
                src = orc.from_ints(field, table)
                t = MLE.new(ctx, n, src)
                tv = np.stack([orc.from_ints(field, tail) for tail in tails]) if n > 1 else np.zeros((np_, 0, 4), dtype=np.uint64)
                got = zk_amd.eq_sums_many(t, tv)
                assert np.array_equal(t.evaluation_slice(), src), (fi, n, np_, "the table changed")
                print("SUMS", fri_ref.FIELD_IDS[fi], "n%d_m%d" % (n, np_), digest(got.tobytes()))
                t.free()
        for n in ref.LINCOMB_VARS:
            for k in ref.LINCOMB_COUNTS:
                tables, coeffs = ref.lincomb_case(fi, n, k, worst_case_values)
                srcs = [orc.from_ints(field, t) for t in tables]
                ts = [MLE.new(ctx, n, s) for s in srcs]
                out = zk_amd.lincomb(ts, orc.from_ints(field, coeffs))
                assert all(np.array_equal(t.evaluation_slice(), s) for t, s in zip(ts, srcs)), (fi, n, k, "a source changed")
                print("LINCOMB", fri_ref.FIELD_IDS[fi], "n%d_k%d" % (n, k), digest(out.evaluation_slice().tobytes()))
                for t in ts + [out]:
                    t.free()
    if setting == "default":   # BN254: expected by the parent from the C oracle's arithmetic
        p = orc.modulus(0)
        for n in ORACLE_SUMS_VARS:
            t = MLE.random(ctxs[0], n, BIG_SEED + n)
            got = zk_amd.eq_sums_many(t, np.stack([orc.from_ints(0, tail) for tail in big_tails(p, n)]))
            print("BIGSUMS", fri_ref.FIELD_IDS[0], "n%d" % n, digest(got.tobytes()))
            t.free()
        n, seeds, coeffs, idx = big_lincomb(p)
        ts = [MLE.random(ctxs[0], n, seed) for seed in seeds]
        before = [t.evaluation_slice().copy() for t in ts]
        out = zk_amd.lincomb(ts, orc.from_ints(0, coeffs))
        assert all(np.array_equal(t.evaluation_slice(), s) for t, s in zip(ts, before)), "a source of the large lincomb changed"
        print("BIGLINCOMB", fri_ref.FIELD_IDS[0], "n%d" % n, digest(np.ascontiguousarray(out.evaluation_slice()[idx]).tobytes()))
        del before
        for t in ts + [out]:
            t.free()
    for case in ref.GPU_CASES:
        n, b, f, q, k, m = case
        fi = ref.case_field(case)
        tables, shift, seed, points = ref.case_inputs(fi, case, worst_case_values)
        ts = [MLE.new(ctxs[fi], n, orc.from_ints(fi, t)) for t in tables]
        com = zk_amd.MultilinearBatchCommitment.commit(ts, b, orc.from_int(fi, shift))
        for t in ts:
            t.free()   # the commitment owns what it needs
        assert (com.n_vars(), com.n_tables()) == (n, k)
        root = com.root()
        pv = np.stack([orc.from_ints(fi, z) for z in points])
        values, proof = com.open(pv, f, q, seed)
        assert zk_amd.mlbatch_verify(fi, root, pv, values, proof, b, f, q, orc.from_int(fi, shift), seed), case
        print("PROOF", fri_ref.FIELD_IDS[fi], case_key(case), digest(root + values.tobytes() + proof))
        com.free()
    for ctx in ctxs:
        ctx.close()
    print(f"mlbatch {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
