"""Run by tests/test_gpu_fri.py in child processes (the library reads its ZK_* switches once per process), and imported by it for the
settings, so that the parent and the children hold the same cases.

  python fri_check.py <setting>    setting: default | fused | binary
      under ZK_FRI_FUSED_FOLD as the parent sets it: a digest of the output of every zk_fri_fold of tests/fri_ref.py's fold cases (each
      input is checked to be left intact) and of every zk_fri_prove of its GPU cases (each proof is given to zk_fri_verify_host); then
      the folds of fri_ref.FOLD_BIG that name this setting and the proofs of fri_ref.PROOF_BIG (big below): one BIG line per check
      with PASS or FAIL, which the parent asserts on, and one BIGPROOF line with the digest of each proof"""
import hashlib
import os
import random
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


def big_fold_key(a, log_n):
    return f"fold_a{a}_n{log_n}"


def _big_fold(ctx, a, log_n):
    """zk_fri_fold of 2^log_n seeded points by 2^a with 2^24 outputs (two sweeps of the capped grid): yields (check, passed, detail)"""
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE

    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    rng = random.Random(0xB16F01D + 64 * a + log_n)
    s, beta = rng.randrange(1, p), rng.randrange(p)
    w = ref.root(field, 1 << log_n)
    sv, bv, swv = orc.from_int(field, s), orc.from_int(field, beta), orc.from_int(field, s * w % p)
    m = 1 << (log_n - a)
    layer = MLE.random(ctx, log_n, 0xF01D0000 + log_n)
    before = layer.clone()
    out = zk_amd.fri_fold(layer, a, sv, bv)
    # every output against outputs that one sweep covers: the fold's even outputs are the fold of the even inputs over the same shift, its
    # odd outputs the fold of the odd inputs over shift * w_N (tests/test_fri_host.py holds this on the definition)
    even, odd = layer.split(2)
    half_even, half_odd = zk_amd.fri_fold(even, a, sv, bv), zk_amd.fri_fold(odd, a, swv, bv)
    joined = MLE.interleave([half_even, half_odd])
    yield "even_odd", joined == out, ""
    yield "input_intact", layer == before, ""
    joined.free()
    before.free()
    v_in, v_out = layer.evaluation_slice(), out.evaluation_slice()

    def sampled(values, get, log_points, shift, indices):
        bad = [i for i in indices if orc.to_int(field, values[i]) != ref.fold_at(field, get, log_points, shift, beta, a, i)]
        return not bad, f"{len(bad)}_of_{len(indices)}_differ_first_{bad[:4]}".replace(" ", "")

    yield ("sampled",) + sampled(v_out, lambda i: orc.to_int(field, v_in[i]), log_n, s, ref.fold_big_samples(m))
    few = ref.fold_big_samples(m >> 1, ref.FOLD_BIG_HALF_SAMPLES)
    yield ("half_even_sampled",) + sampled(half_even.evaluation_slice(), lambda i: orc.to_int(field, v_in[2 * i]), log_n - 1, s, few)
    yield ("half_odd_sampled",) + sampled(half_odd.evaluation_slice(), lambda i: orc.to_int(field, v_in[2 * i + 1]), log_n - 1, s * w % p, few)
    for t in (layer, out, even, odd, half_even, half_odd):
        t.free()


def _big_proof(ctx, case, emit):
    """one proof whose layer 0 has 2^22 points: yields (check, passed, detail); emit(digest of the proof)"""
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MerkleTree
    from zk_amd import UnivariatePolynomial as Poly

    field = zk_amd.BN254_FR
    d, b, a, f, q = case
    p = orc.modulus(field)
    rng = random.Random(0xB16 + ref.hash_case(case))
    shift = rng.randrange(1, p)
    sv = orc.from_int(field, shift)
    seed = bytes(rng.randrange(256) for _ in range(32))
    poly = Poly.new(ctx, orc.fill_random(field, 0xC0EF + a, 1 << d))
    proof = zk_amd.fri_prove(poly, *case, sv, seed)
    emit(digest(proof))
    yield "length", len(proof) == ref.proof_bytes(*case), ""
    yield "host_verifier_accepts", zk_amd.fri_verify(field, proof, *case, sv, seed), ""
    yield "definition_accepts", ref.verify(field, proof, *case, shift, seed), ""
    flipped = bytearray(proof)
    flipped[len(proof) // 3] ^= 2
    yield "flipped_byte_rejected", not zk_amd.fri_verify(field, bytes(flipped), *case, sv, seed) and not ref.verify(field, bytes(flipped), *case, shift, seed), ""
    yield "wrong_seed_rejected", not zk_amd.fri_verify(field, proof, *case, sv, bytes(32)) and not ref.verify(field, proof, *case, shift, bytes(32)), ""
    # the first root: the commitment to the 2^a column views of the LDE (contiguous parts: variable 0 is the most significant index bit)
    lde = zk_amd.fri_lde(poly, d + b, sv)
    views = [lde.partial_evaluate(0, orc.from_ints(field, [(j >> (a - 1 - t)) & 1 for t in range(a)])) for j in range(1 << a)]
    tree = MerkleTree.commit(views)
    yield "first_root_is_the_commitment_to_the_lde", tree.root() == proof[:32], ""
    # and the same root by the bulk reference over the downloaded LDE: the commitment above runs the prover's own kernels
    images = np.frombuffer(orc.mle_to_bytes(field, d + b, lde.evaluation_slice()), dtype=np.uint8).reshape(1 << a, 1 << (d + b - a), 32)
    yield "first_root_is_the_reference_root_of_the_lde", ref.merkle_ref.commit_bulk(list(images))[-1] == proof[:32], ""
    tree.free()
    for t in views + [lde]:
        t.free()
    poly.free()


def big(setting):
    """never raises: a check that does not hold, or a call that fails, is a FAIL line, so that the cases above stay judged on their own"""
    import zk_amd

    def run(key, checks):
        try:
            for name, passed, detail in checks:
                print("BIG", key, name, "PASS" if passed else "FAIL", detail, flush=True)
        except Exception as e:   # noqa: BLE001
            print("BIG", key, "completed", "FAIL", repr(e).replace(" ", "_"), flush=True)
        else:
            print("BIG", key, "completed", "PASS", flush=True)

    ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
    for a, log_n, settings in ref.FOLD_BIG:
        if setting in settings:
            run(big_fold_key(a, log_n), _big_fold(ctx, a, log_n))
    for case in ref.PROOF_BIG:
        run(case_key(case), _big_proof(ctx, case, lambda dg, case=case: print("BIGPROOF", case_key(case), dg, flush=True)))
    ctx.close()


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
    big(setting)
    print(f"fri {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
