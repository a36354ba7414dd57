"""Run by tests/test_gpu_pcs_large.py in child processes (the library reads its ZK_* switches once per process), and imported by it for
the settings, so that the parent and the children hold the same cases (tests/pcs_ref.py, "the shapes of tests/test_gpu_pcs_large.py").

  python pcs_large_check.py <setting>    setting: default | fused | binary
      under ZK_FRI_FUSED_FOLD as the parent sets it: a digest of the root, the values and the proof of every mid opening (with the
      verdict of zk_pcs_verify_host on it); in the default child also of every wide opening and of the output of every wide and every edge
      zk_deep_quotient (the columns are checked to be left intact), then the big quotients and the big opening (big below): one BIG
      line per check with PASS or FAIL, which the parent asserts on.  TIME lines give the seconds of each part (for the record only)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fri_ref  # noqa: E402
import pcs_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from pcs_check import SETTINGS, SWITCH, case_key, digest, quotient_key  # noqa: E402,F401


def big_quotient_key(log_n, k):
    return f"quotient_n{log_n}_k{k}"


def _big_quotient(ctx, log_n, k):
    """zk_deep_quotient of k seeded columns of 2^log_n points, more chunk products than k_pcs_totals has threads: yields (check, passed,
    detail)"""
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE

    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    s, z, alpha, ys = ref.big_quotient_inputs(log_n, k)
    sw = s * fri_ref.root(field, 1 << log_n) % p
    sv, swv, zv, av, yv = orc.from_int(field, s), orc.from_int(field, sw), orc.from_int(field, z), orc.from_int(field, alpha), orc.from_ints(field, ys)
    cols = [MLE.random(ctx, log_n, 0xDEE90000 + 64 * log_n + c) for c in range(k)]
    before = [col.clone() for col in cols]
    out = zk_amd.deep_quotient(cols, sv, zv, yv, av)
    # every output against outputs of half the size: x_{2i} = s (w^2)^i and x_{2i+1} = (s w) (w^2)^i, so the even outputs are the quotient
    # of the even rows over the coset of s and the odd outputs that of the odd rows over the coset of s w_N, with the same z, values
    # and alpha (tests/test_pcs_large_host.py holds this on the definition)
    halves = [col.split(2) for col in cols]
    half_even = zk_amd.deep_quotient([h[0] for h in halves], sv, zv, yv, av)
    half_odd = zk_amd.deep_quotient([h[1] for h in halves], swv, zv, yv, av)
    joined = MLE.interleave([half_even, half_odd])
    yield "even_odd", joined == out, ""
    yield "input_intact", all(col == b for col, b in zip(cols, before)), ""
    joined.free()
    for t in before + [t for h in halves for t in h]:
        t.free()
    v_cols, v_out = [col.evaluation_slice() for col in cols], out.evaluation_slice()

    def sampled(values, row_of, log_points, shift, indices):
        """values[i] against quotient_at on the rows v_cols[c][row_of(i)]"""
        at = np.array(indices, dtype=np.int64)
        got = orc.to_ints(field, values[at])
        rows = [dict(zip(indices, orc.to_ints(field, v[row_of(at)]))) for v in v_cols]
        bad = [i for i, g in zip(indices, got) if g != ref.quotient_at(field, lambda c, j: rows[c][j], k, log_points, shift, z, ys, alpha, i)]
        return not bad, f"{len(bad)}_of_{len(indices)}_differ_first_{bad[:4]}".replace(" ", "")

    yield ("sampled",) + sampled(v_out, lambda i: i, log_n, s, ref.quotient_big_samples(log_n))
    few = ref.quotient_big_samples(log_n - 1, ref.BIG_HALF_SAMPLES)
    yield ("half_even_sampled",) + sampled(half_even.evaluation_slice(), lambda i: 2 * i, log_n - 1, s, few)
    yield ("half_odd_sampled",) + sampled(half_odd.evaluation_slice(), lambda i: 2 * i + 1, log_n - 1, sw, few)
    for t in cols + [out, half_even, half_odd]:
        t.free()


def _big_opening(ctx):
    """the opening ref.BIG_CASE, two polynomials of 2^19 and 2^19 - 1 coefficients: yields (check, passed, detail)"""
    import zk_amd
    from oracle import binding as orc
    from zk_amd import UnivariatePolynomial as Poly

    field = zk_amd.BN254_FR
    case = ref.BIG_CASE
    k, d, b, a, f, q = case
    p = orc.modulus(field)
    shift, seed, z, other_z = ref.big_case_inputs()
    sv = orc.from_int(field, shift)
    coeffs = [orc.fill_random(field, 0xC0EF19 + c, (1 << d) - c) for c in range(k)]
    handles = [Poly.new(ctx, co) for co in coeffs]
    com = zk_amd.PolyCommitment.commit(handles, d, b, a, sv)
    for h in handles:
        h.free()
    root = com.root()
    values, proof = com.open(orc.from_int(field, z), f, q, seed)
    com.free()
    yield "length", len(proof) == ref.proof_bytes(*case), ""
    ints = [orc.to_ints(field, co) for co in coeffs]
    ys = [ref.evaluate(field, co, z) for co in ints]
    yield "values", orc.to_ints(field, values) == ys, ""
    # the root from the LDEs by the oracle's transform: nothing of it comes from the device
    images = []
    for co in ints:
        lde = ref.lde_by_oracle(field, co, d + b, shift)
        images += list(np.frombuffer(orc.mle_to_bytes(field, d + b, lde), dtype=np.uint8).reshape(1 << a, 1 << (d + b - a), 32))
    want_root = ref.merkle_ref.commit_bulk(images)[-1]
    yield "root", root == want_root, ""

    def host(at, vals, pr):
        return zk_amd.pcs_verify(field, root, orc.from_int(field, at), vals, pr, d, b, a, f, q, sv, seed)

    def definition(at, vals, pr):
        return ref.verify(field, k, d, b, a, f, q, shift, seed, want_root, at, vals, pr)

    yield "host_verifier_accepts", host(z, values, proof), ""
    yield "definition_accepts", definition(z, ys, proof), ""
    yield "other_z_rejected", not host(other_z, values, proof) and not definition(other_z, ys, proof), ""
    changed = list(ys)
    changed[1] = (changed[1] + 1) % p
    yield "changed_value_rejected", not host(z, orc.from_ints(field, changed), proof) and not definition(z, changed, proof), ""
    # the low byte of element 5 of the commitment row of query q / 2 (the rows and paths of the commitment follow the FRI part)
    width, log_m = k << a, d + b - a
    flipped = bytearray(proof)
    flipped[fri_ref.proof_bytes(d, b, a, f, q) + (q // 2) * 32 * (width + log_m) + 32 * 5 + 31] ^= 2
    yield "flipped_row_byte_rejected", not host(z, values, bytes(flipped)) and not definition(z, ys, bytes(flipped)), ""


def big():
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
    for log_n, k in ref.BIG_QUOTIENTS:
        t0 = time.perf_counter()
        run(big_quotient_key(log_n, k), _big_quotient(ctx, log_n, k))
        print("TIME", big_quotient_key(log_n, k), f"{time.perf_counter() - t0:.2f}", flush=True)
    t0 = time.perf_counter()
    run(case_key(ref.BIG_CASE), _big_opening(ctx))
    print("TIME", case_key(ref.BIG_CASE), f"{time.perf_counter() - t0:.2f}", flush=True)
    ctx.close()


def check(setting):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd import UnivariatePolynomial as Poly

    assert os.environ.get(SWITCH) == SETTINGS[setting].get(SWITCH), os.environ.get(SWITCH)
    t0 = time.perf_counter()
    fields = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)
    ctxs = [zk_amd.Context(field, 0) for field in fields]
    for fi, field in enumerate(fields):
        ctx, p = ctxs[fi], orc.modulus(field)
        for n_vars in (0, 1, 4, 8, 10, 12, 14, 16, 17):   # stale pool data in the size classes of the tables
            MLE.random(ctx, n_vars, 900 + n_vars).free()
        if setting != "default":
            continue
        for log_n, k in ref.wide_quotient_sizes(fi) + ref.edge_quotient_sizes(fi):
            src = [orc.from_ints(field, col) for col in ref.quotient_columns(p, fi, log_n, k, worst_case_values)]
            cols = [MLE.new(ctx, log_n, s) for s in src]
            for shift_name, zi, ai in ref.THINNED_COMBOS:
                s, z, alpha, ys = ref.quotient_case(fi, log_n, k, shift_name, zi, ai)
                out = zk_amd.deep_quotient(cols, orc.from_int(field, s), orc.from_int(field, z), orc.from_ints(field, ys), orc.from_int(field, alpha))
                print("QUO", fri_ref.FIELD_IDS[fi], quotient_key(log_n, k, shift_name, zi, ai), digest(out.evaluation_slice().tobytes()))
                out.free()
            for col, s in zip(cols, src):
                assert np.array_equal(col.evaluation_slice(), s), (fi, log_n, k, "a column changed")
                col.free()
    print("TIME", "quotients", f"{time.perf_counter() - t0:.2f}", flush=True)
    t0 = time.perf_counter()
    for fi, case in ref.MID_CASES + (ref.WIDE_CASES if setting == "default" else ()):
        k, d, b, a, f, q = case
        polys, shift, seed, z = ref.case_inputs(fi, case)
        handles = [Poly.new(ctxs[fi], orc.from_ints(fi, co)) for co in polys]
        com = zk_amd.PolyCommitment.commit(handles, d, b, a, orc.from_int(fi, shift))
        for h in handles:   # the commitment owns what it needs
            h.free()
        root = com.root()
        values, proof = com.open(orc.from_int(fi, z), f, q, seed)
        ok = zk_amd.pcs_verify(fi, root, orc.from_int(fi, z), values, proof, d, b, a, f, q, orc.from_int(fi, shift), seed)
        print("PROOF", fri_ref.FIELD_IDS[fi], case_key(case), digest(root + values.tobytes() + proof), "accepted" if ok else "REJECTED", flush=True)
        com.free()
    print("TIME", "openings", f"{time.perf_counter() - t0:.2f}", flush=True)
    for ctx in ctxs:
        ctx.close()
    if setting == "default":
        big()
    print(f"pcs large {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
