"""Run by tests/test_gpu_perm.py in child processes, and imported by it for the case lists, so that parent and child hold the same cases.

  python perm_check.py [all|fused]
      per case of tests/perm_ref.py's GPU list (fused: the cases whose tree has a launch above the LDS stage, which is where the
      switches ZK_PERM_FUSE, ZK_GPROD_TREE_FUSE and ZK_PERM_MAX_GRID select another kernel) a digest of proof, point and claims of
      zk_perm_prove with zk_perm_verify_host's verdict, and a digest of zk_mle_perm_fingerprint's table; zk_gprod_prove on that table
      under seed' is checked to give the head of the proof, and the columns are checked to be left intact"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gprod_ref  # noqa: E402
import perm_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

FIELD_IDS = ("bn254", "bls12_381", "bls12_377")


def digest(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def check(which):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE

    fields = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)
    ctxs = [zk_amd.Context(field, 0) for field in fields]
    for ctx in ctxs:
        for n_vars in (0, 1, 4, 8, 10, 12, 14):   # stale pool data in the size classes of the scratch
            MLE.random(ctx, n_vars, 900 + n_vars).free()
    for case in (ref.GPU_FUSED_CASES if which == "fused" else ref.GPU_CASES):
        n, k = case[0], case[1]
        fi, w, sigma, beta, gamma, seed = ref.case_inputs(case, worst_case_values)
        ctx = ctxs[fi]
        srcs = [orc.from_ints(fi, t) for t in list(w) + list(sigma)]
        tabs = [MLE.new(ctx, n, s) for s in srcs]
        bv, gv = orc.from_int(fi, beta), orc.from_int(fi, gamma)
        proof, point, claims = zk_amd.permutation_prove(tabs[:k], tabs[k:], bv, gv, seed)
        got = zk_amd.permutation_verify(fi, n, k, bv, gv, seed, proof)
        assert got is None or (np.array_equal(got[0], point) and np.array_equal(got[1], claims)), case
        print("PROOF", FIELD_IDS[fi], ref.case_key(case), digest(proof + point.tobytes() + claims.tobytes()), int(got is not None))
        fp = zk_amd.perm_fingerprint(tabs[:k], tabs[k:], bv, gv)
        N = ref.total_vars(n, k)
        assert fp.n_vars() == N, case
        print("FP", FIELD_IDS[fi], ref.case_key(case), digest(fp.evaluation_slice().tobytes()), 0)
        # the grand product of the materialised table under seed' is the head of the proof: no reference needed
        _, head, gpoint, _ = zk_amd.grand_product_prove(fp, ref.seed_prime(fi, n, k, beta, gamma, seed))
        assert head == proof[:gprod_ref.proof_bytes(N)], case
        kp = ref.kappa(k)
        assert np.array_equal(gpoint[kp:kp + n], point), case
        print("HEAD", FIELD_IDS[fi], ref.case_key(case), digest(head), 0)
        fp.free()
        for t, s in zip(tabs, srcs):
            assert np.array_equal(t.evaluation_slice(), s), (case, "a column changed")
            t.free()
    for ctx in ctxs:
        ctx.close()
    print("perm ok")


if __name__ == "__main__":
    check(sys.argv[1] if len(sys.argv) > 1 else "all")
