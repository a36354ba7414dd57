"""Run by tests/test_gpu_fri.py in child processes (the library reads its ZK_* switches once per process), and imported by it for the
settings, so that the parent and the children hold the same cases.

  python fri_check.py <setting>    setting: default | fused | binary
      under ZK_FRI_FUSED_FOLD as the parent sets it: a digest of the output of every zk_fri_fold of tests/fri_ref.py's fold cases (each
      input is checked to be left intact) and of every zk_fri_prove of its GPU cases (each proof is given to zk_fri_verify_host)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fri_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

SWITCH = "ZK_FRI_FUSED_FOLD"
# fused: one launch of k_fri_fold<a> per layer; binary: a launches of k_fri_fold<1>; default: what ships
SETTINGS = {"default": {}, "fused": {SWITCH: "1"}, "binary": {SWITCH: "0"}}


def digest(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def fold_key(a, log_n, shift_name, beta_index):
    return f"a{a}_n{log_n}_{shift_name}_b{beta_index}"


def case_key(case):
    return "d%d_b%d_a%d_f%d_q%d" % case


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
        for n_vars in (0, 1, 4, 8, 10, 12, 14):   # stale pool data in the size classes of the layers
            MLE.random(ctx, n_vars, 700 + n_vars).free()
        for a, log_n in ref.fold_cases(fi):
            src = orc.from_ints(field, ref.fold_input(p, fi, log_n, worst_case_values))
            layer = MLE.new(ctx, log_n, src)
            betas = ref.fold_betas(p, fi, a, log_n)
            for shift_name, k in ref.fold_combos(log_n):
                out = zk_amd.fri_fold(layer, a, orc.from_int(field, ref.shift_value(p, shift_name)), orc.from_int(field, betas[k]))
                print("FOLD", ref.FIELD_IDS[fi], fold_key(a, log_n, shift_name, k), digest(out.evaluation_slice().tobytes()))
                out.free()
            assert np.array_equal(layer.evaluation_slice(), src), (fi, a, log_n, "the input changed")
            layer.free()
    for case in ref.GPU_CASES:
        fi = ref.case_field(case)
        coeffs, shift, seed = ref.case_inputs(fi, case)
        poly = Poly.new(ctxs[fi], orc.from_ints(fi, coeffs))
        proof = zk_amd.fri_prove(poly, *case, orc.from_int(fi, shift), seed)
        assert zk_amd.fri_verify(fi, proof, *case, orc.from_int(fi, shift), seed), case
        print("PROOF", ref.FIELD_IDS[fi], case_key(case), digest(proof))
        poly.free()
    for ctx in ctxs:
        ctx.close()
    print(f"fri {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
