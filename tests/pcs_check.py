"""Run by tests/test_gpu_pcs.py in child processes (the library reads its ZK_* switches once per process), and imported by it for the
settings, so that the parent and the children hold the same cases.

  python pcs_check.py <setting>    setting: default | fused | binary
      under ZK_FRI_FUSED_FOLD as the parent sets it (the only switch on the commitment's path; the quotient has none): a digest of the
      values and the proof of every opening of tests/pcs_ref.py's GPU cases (each proof is given to zk_pcs_verify_host) and, in the default
      child, of the output of every zk_deep_quotient of its quotient cases (the columns are checked to be left intact)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fri_ref  # noqa: E402
import pcs_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

SWITCH = "ZK_FRI_FUSED_FOLD"
SETTINGS = {"default": {}, "fused": {SWITCH: "1"}, "binary": {SWITCH: "0"}}


def digest(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def quotient_key(log_n, k, shift_name, zi, ai):
    return f"n{log_n}_k{k}_{shift_name}_z{zi}_a{ai}"


def case_key(case):
    return "k%d_d%d_b%d_a%d_f%d_q%d" % case


def check(setting):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd import UnivariatePolynomial as Poly

    assert os.environ.get(SWITCH) == SETTINGS[setting].get(SWITCH), os.environ.get(SWITCH)
    fields = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)
    ctxs = [zk_amd.Context(field, 0) for field in fields]
    for fi, field in enumerate(fields):
        ctx, p = ctxs[fi], orc.modulus(field)
        for n_vars in (0, 1, 4, 8, 10, 12, 14, 16):   # stale pool data in the size classes of the tables
            MLE.random(ctx, n_vars, 900 + n_vars).free()
        if setting != "default":
            continue
        for log_n, k in ref.quotient_sizes(fi):
            src = [orc.from_ints(field, col) for col in ref.quotient_columns(p, fi, log_n, k, worst_case_values)]
            cols = [MLE.new(ctx, log_n, s) for s in src]
            for shift_name, zi, ai in ref.quotient_combos(log_n, k):
                s, z, alpha, ys = ref.quotient_case(fi, log_n, k, shift_name, zi, ai)
                out = zk_amd.deep_quotient(cols, orc.from_int(field, s), orc.from_int(field, z), orc.from_ints(field, ys), orc.from_int(field, alpha))
                print("QUO", fri_ref.FIELD_IDS[fi], quotient_key(log_n, k, shift_name, zi, ai), digest(out.evaluation_slice().tobytes()))
                out.free()
            for col, s in zip(cols, src):
                assert np.array_equal(col.evaluation_slice(), s), (fi, log_n, k, "a column changed")
                col.free()
    for case in ref.GPU_CASES:
        k, d, b, a, f, q = case
        fi = ref.case_field(case)
        polys, shift, seed, z = ref.case_inputs(fi, case)
        handles = [Poly.new(ctxs[fi], orc.from_ints(fi, co)) for co in polys]
        com = zk_amd.PolyCommitment.commit(handles, d, b, a, orc.from_int(fi, shift))
        for h in handles:   # the commitment owns what it needs
            h.free()
        root = com.root()
        values, proof = com.open(orc.from_int(fi, z), f, q, seed)
        assert zk_amd.pcs_verify(fi, root, orc.from_int(fi, z), values, proof, d, b, a, f, q, orc.from_int(fi, shift), seed), case
        print("PROOF", fri_ref.FIELD_IDS[fi], case_key(case), digest(root + values.tobytes() + proof))
        com.free()
    for ctx in ctxs:
        ctx.close()
    print(f"pcs {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
