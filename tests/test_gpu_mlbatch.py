"""zk_mlbatch_commit / zk_mlbatch_open / zk_mlbatch_verify_host / zk_mle_lincomb / zk_mle_eq_sums_many / zk_bench_mlbatch on the device.
The reference has no polynomial commitment: tests/mlbatch_ref.py is the definition.  In child processes under ZK_MLBATCH_FUSE_FOLD (the
switch between the combine-and-fold kernel and the linear combination into a scratch layer with FRI's fold): every opening of the shared
case list -- root, values and proof -- byte for byte against the definition, on every setting; in the default child every
zk_mle_eq_sums_many and zk_mle_lincomb case against Python integers, on BN254 the multi-point sums at the run length 2^9 and at the
smallest table whose capped grid takes a second trip against the C oracle's arithmetic, and the lincomb whose grid-stride loop takes a
second trip on sampled outputs.  In the parent several openings of one handle, a lookup and a two-point argument settled by one opening
each, the error table, the measurement hook and the C++ mirror."""
import os
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd._lib import c, lib, u8p, u64p

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_ref  # noqa: E402
import mlbatch_ref as ref  # noqa: E402
import mlpcs_ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from mlbatch_check import (BIG_SEED, ORACLE_SUMS_VARS, SETTINGS, SUMS_POINTS, SWITCH, big_lincomb, big_tails, case_key,  # noqa: E402
                           digest)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "mlbatch_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
NO_ROOT, BAD, MISMATCH = -7, -20, -26
KINDS = ("SUMS", "BIGSUMS", "LINCOMB", "BIGLINCOMB", "PROOF")


@pytest.fixture(scope="module")
def children():
    """{setting: {(kind, field id, key): digest}}: one child process per switch setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"mlbatch {setting} ok" in r.stdout
        lines = [ln.split() for ln in r.stdout.splitlines()]
        out[setting] = {(ln[0], ln[1], ln[2]): ln[3] for ln in lines if ln and ln[0] in KINDS}
    return out


@pytest.fixture(scope="module")
def expected_proofs():
    """{("PROOF", field id, key): digest of root + values + proof} from the definition, which also accepts each of them"""
    out = {}
    for case in ref.GPU_CASES:
        n, b, f, q, k, m = case
        fi = ref.case_field(case)
        tables, shift, seed, points = ref.case_inputs(fi, case, worst_case_values)
        committed = ref.commit(fi, tables, b, shift)
        root = ref.merkle_ref.root(committed[2])
        values, proof = ref.prove(fi, tables, b, f, q, shift, seed, points, committed=committed)
        assert ref.verify(fi, n, b, f, q, k, shift, seed, root, points, values, proof), case   # the same bytes as the device's, below
        flat = orc.from_ints(fi, [x for row in values for x in row])
        out[("PROOF", fri_ref.FIELD_IDS[fi], case_key(case))] = digest(root + np.ascontiguousarray(flat).tobytes() + proof)
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_opening_on_every_setting(children, expected_proofs, setting):
    """root, values (= t_c(z_j)) and proof of zk_mlbatch_commit / zk_mlbatch_open against mlbatch_ref.prove, byte for byte, by default,
    with the scratch layer and with the combine-and-fold kernel; zk_mlbatch_verify_host accepted each in the child, mlbatch_ref.verify in
    the fixture"""
    got = {key: dg for key, dg in children[setting].items() if key[0] == "PROOF"}
    assert len(expected_proofs) == len(ref.GPU_CASES) and set(got) == set(expected_proofs)
    wrong = sorted(key for key, want in expected_proofs.items() if got[key] != want)
    assert not wrong, (setting, wrong[:20], len(wrong))


def test_eq_sums_many_against_python_integers(children):
    """zk_mle_eq_sums_many on all three fields at every size of mlpcs_ref.EQ_SUMS_VARS with 1, POINTS_PER_PASS and POINTS_PER_PASS + 1
    points; the other children run none (the call has no switch)"""
    got = {key: dg for key, dg in children["default"].items() if key[0] == "SUMS"}
    want = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for n in mlpcs_ref.EQ_SUMS_VARS:
            for np_ in SUMS_POINTS:
                table, tails = ref.eq_sums_many_case(fi, n, np_, worst_case_values)
                if n >= 8:
                    assert {0, 1, p - 1} <= set(tails[0])
                sums = [x for pair in ref.eq_sums_many(table, tails, p) for x in pair]
                want[("SUMS", fri_ref.FIELD_IDS[fi], "n%d_m%d" % (n, np_))] = digest(np.ascontiguousarray(orc.from_ints(field, sums)).tobytes())
    assert set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, wrong
    assert not any(key[0] != "PROOF" for setting in ("unfused", "fused") for key in children[setting])


@pytest.mark.parametrize("n", ORACLE_SUMS_VARS)
def test_eq_sums_many_against_the_oracle(children, n):
    """BN254 with two points at n = 21 (runs of 2^9 elements) and at n = 24, where 2^14 runs meet the capped grid's 2^13 waves and the
    loop takes a second trip.  The expected sums are the C oracle's: its generator's table, each half evaluated at each tail"""
    field = FIELDS[0]
    assert mlpcs_ref.trips(mlpcs_ref.SECOND_TRIP_VARS) == 2 and mlpcs_ref.SECOND_TRIP_VARS in ORACLE_SUMS_VARS
    table = orc.fill_random(field, BIG_SEED + n, 1 << n)
    half = 1 << (n - 1)
    want = np.stack([orc.mle_evaluate(field, n - 1, table[x * half:(x + 1) * half], orc.from_ints(field, tail))
                     for tail in big_tails(orc.modulus(field), n) for x in range(2)])
    assert children["default"][("BIGSUMS", fri_ref.FIELD_IDS[0], "n%d" % n)] == digest(np.ascontiguousarray(want, dtype=np.uint64).tobytes())


def test_lincomb_against_python_integers(children):
    """zk_mle_lincomb on all three fields, k in {1, 2, 3, 8}, n = 0, 1, 5, 6, 7, 13 in full; coefficients in {0, 1, p - 1, random}; the
    child checked that every source was left bit-identical"""
    got = {key: dg for key, dg in children["default"].items() if key[0] == "LINCOMB"}
    want = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        kinds = set()
        for n in ref.LINCOMB_VARS:
            for k in ref.LINCOMB_COUNTS:
                tables, coeffs = ref.lincomb_case(fi, n, k, worst_case_values)
                kinds |= {x if x in (0, 1, p - 1) else "random" for x in coeffs}
                want[("LINCOMB", fri_ref.FIELD_IDS[fi], "n%d_k%d" % (n, k))] = digest(
                    np.ascontiguousarray(orc.from_ints(field, ref.lincomb(tables, coeffs, p))).tobytes())
        assert kinds == {0, 1, p - 1, "random"}
    assert set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, wrong


def test_lincomb_second_trip(children):
    """BN254, k = 3, 2^23 elements: 2^22 threads take one element per trip, so every thread takes a second trip.  4096 seeded sample
    indices, the first and last 64 elements and both sides of the trip boundary against Python integers over the oracle's generator"""
    field = FIELDS[0]
    p = orc.modulus(field)
    n, seeds, coeffs, idx = big_lincomb(p)
    assert n == ref.LINCOMB_SECOND_TRIP_VARS and ref.lincomb_trips(n) == 2 and ref.lincomb_trips(n - 1) == 1 and len(seeds) == 3
    assert set(range(64)) <= set(idx) and set(range((1 << n) - 64, 1 << n)) <= set(idx) and len(idx) >= 4096 + 128
    rows = [orc.to_ints(field, np.ascontiguousarray(orc.fill_random(field, seed, 1 << n)[idx])) for seed in seeds]
    want = [sum(cf * row[i] for cf, row in zip(coeffs, rows)) % p for i in range(len(idx))]
    assert children["default"][("BIGLINCOMB", fri_ref.FIELD_IDS[0], "n%d" % n)] == digest(np.ascontiguousarray(orc.from_ints(field, want)).tobytes())


@pytest.fixture(params=range(3), ids=fri_ref.FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def _points(field, points):
    return np.stack([orc.from_ints(field, z) for z in points])


def test_many_openings_of_one_handle(fctx):
    """the handle survives an open: three different point sets, one of them again, give the definition's bytes, then another (f, Q); the
    root is unchanged; the source tables may be freed after the commitment and are bit-identical when they are kept; the handle's blocks
    are cut from stale pool data, not zeros"""
    fi, field, ctx = fctx
    p = orc.modulus(field)
    case = (10, 2, 1, 8, 3, 2)
    n, b, f, q, k, m = case
    tables, shift, seed, z1 = ref.case_inputs(fi, case, worst_case_values)
    sv, srcs = orc.from_int(field, shift), [orc.from_ints(field, t) for t in tables]
    for n_vars in (9, 10, 11, 12, 13):
        MLE.random(ctx, n_vars, 77 + n_vars).free()
    kept, gone = [MLE.new(ctx, n, s) for s in srcs], [MLE.new(ctx, n, s) for s in srcs]
    com = zk_amd.MultilinearBatchCommitment.commit(gone, b, sv)
    for t in gone:
        t.free()
    com_kept = zk_amd.MultilinearBatchCommitment.commit(kept, b, sv)
    assert all(np.array_equal(t.evaluation_slice(), s) for t, s in zip(kept, srcs))
    assert (com.n_vars(), com.n_tables()) == (n, k)
    committed = ref.commit(field, tables, b, shift)
    root = com.root()
    assert root == ref.merkle_ref.root(committed[2]) == com_kept.root()
    z2 = [[(7 * x + 3) % p for x in z] for z in z1]
    z3 = [z1[1], z2[0], z1[1]]                                # three points, two of them equal
    for zs in (z1, z2, z3, z1):
        values, proof = com.open(_points(field, zs), f, q, seed)
        want_v, want = ref.prove(field, tables, b, f, q, shift, seed, zs, committed=committed)
        assert [orc.to_ints(field, row) for row in values] == want_v and proof == want, zs
        assert len(proof) == zk_amd.mlbatch_proof_bytes(n, k, len(zs), b, f, q)
        assert zk_amd.mlbatch_verify(field, root, _points(field, zs), values, proof, b, f, q, sv, seed)
        zb = [[(zs[0][0] + 1) % p] + list(zs[0][1:])] + [list(z) for z in zs[1:]]
        assert not zk_amd.mlbatch_verify(field, root, _points(field, zb), values, proof, b, f, q, sv, seed)
    assert com.root() == root
    values, proof = com_kept.open(_points(field, z2), 4, 3, seed)   # another final length and query count
    want_v, want = ref.prove(field, tables, b, 4, 3, shift, seed, z2, committed=committed)
    assert [orc.to_ints(field, row) for row in values] == want_v and proof == want
    assert all(np.array_equal(t.evaluation_slice(), s) for t, s in zip(kept, srcs)) and com_kept.root() == root
    com.free()
    com_kept.free()


def test_a_lookup_settled_by_one_opening():
    """lookup_prove on a witness of 2^9 entries over a table of 2^6, `table` and `m` in ONE batch commitment: m comes from
    lookup_multiplicities before alpha is drawn, the seed binds the roots, and lookup_verify's (r_t, t_claim, m_claim) are settled by one
    open at r_t; with m_claim + 1 the batch verifier rejects"""
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx = zk_amd.Context(field, 0)
    rng = np.random.default_rng(17)
    table_vals = orc.fill_random(field, 4242, 1 << 6)
    table = MLE.new(ctx, 6, table_vals)
    witness = MLE.new(ctx, 9, table_vals[rng.integers(0, 1 << 6, 1 << 9)])
    m, missing, _, _ = zk_amd.lookup_multiplicities(table, witness)
    assert missing == 0
    b, f, q = 1, 2, 8
    shift = orc.from_int(field, 5)
    com = zk_amd.MultilinearBatchCommitment.commit([table, m], b, shift)
    com_w = zk_amd.MultilinearCommitment.commit(witness, b, shift)
    seed = zk_amd.keccak256(com.root() + com_w.root())                       # binds the roots before any challenge exists
    alpha = orc.from_int(field, int.from_bytes(zk_amd.keccak256(seed + b"alpha"), "big") % p)
    m2, proof = zk_amd.lookup_prove(witness, table, alpha, seed)
    assert np.array_equal(m2.evaluation_slice(), m.evaluation_slice())
    got = zk_amd.lookup_verify(field, 9, 6, alpha, seed, proof)
    assert got is not None
    (r_f, f_claim), (r_t, t_claim, m_claim) = got
    values, opening = com.open(r_t[None], f, q, seed)
    assert values.shape == (1, 2, 4) and np.array_equal(values[0, 0], t_claim) and np.array_equal(values[0, 1], m_claim)
    claimed = np.stack([t_claim, m_claim])[None]
    assert zk_amd.mlbatch_verify(field, com.root(), r_t[None], claimed, opening, b, f, q, shift, seed)
    wrong = claimed.copy()
    wrong[0, 1] = orc.from_int(field, (orc.to_int(field, m_claim) + 1) % p)
    assert not zk_amd.mlbatch_verify(field, com.root(), r_t[None], wrong, opening, b, f, q, shift, seed)
    v_w, open_w = com_w.open(r_f, f, q, seed)                                  # the witness has another size: its own commitment
    assert np.array_equal(v_w, f_claim) and zk_amd.mlpcs_verify(field, com_w.root(), r_f, f_claim, open_w, b, f, q, shift, seed)
    for h in (com, com_w):
        h.free()
    ctx.close()


def test_two_arguments_settled_by_one_opening_at_two_points():
    """k = 3 columns under one commitment; grand_product_prove on a challenge-weighted sum of them (lincomb) leaves a claim at r1,
    fractional_sum_prove on the same sum one at r2; ONE open at {r1, r2}; the verifier recombines the 3 values per point with the same
    weights and compares them with the two claims"""
    field = zk_amd.BLS12_381_FR
    p = orc.modulus(field)
    ctx = zk_amd.Context(field, 0)
    n, b, f, q = 8, 1, 1, 8
    cols = [MLE.random(ctx, n, 600 + j) for j in range(3)]
    shift = orc.from_int(field, 5)
    com = zk_amd.MultilinearBatchCommitment.commit(cols, b, shift)
    root = com.root()
    seed = zk_amd.keccak256(root)                                              # the weights are drawn after the root
    w = [int.from_bytes(zk_amd.keccak256(seed + bytes([j])), "big") % p for j in range(3)]
    mix = zk_amd.lincomb(cols, orc.from_ints(field, w))
    host_cols = [orc.to_ints(field, t.evaluation_slice()) for t in cols]
    assert orc.to_ints(field, mix.evaluation_slice()) == ref.lincomb(host_cols, w, p)
    seed1, seed2 = zk_amd.keccak256(seed + b"gprod"), zk_amd.keccak256(seed + b"fsum")
    product, proof1, _, _ = zk_amd.grand_product_prove(mix, seed1)
    total, proof2, _, _ = zk_amd.fractional_sum_prove(mix, seed2)
    got1 = zk_amd.grand_product_verify(field, n, seed1, product, proof1)
    got2 = zk_amd.fractional_sum_verify(field, n, False, seed2, total, proof2)
    assert got1 is not None and got2 is not None
    (r1, claim1), (r2, claims2) = got1, got2
    points = np.stack([r1, r2])
    values, opening = com.open(points, f, q, seed)
    assert values.shape == (2, 3, 4)
    assert zk_amd.mlbatch_verify(field, root, points, values, opening, b, f, q, shift, seed)
    for j, claim in enumerate((claim1, claims2[1])):
        assert sum(wc * v for wc, v in zip(w, orc.to_ints(field, values[j]))) % p == orc.to_int(field, claim), j
    swapped = values[::-1].copy()                                              # the values of the two points exchanged
    assert not zk_amd.mlbatch_verify(field, root, points, swapped, opening, b, f, q, shift, seed)
    com.free()
    ctx.close()


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    n, k = 6, 3
    ts = [MLE.random(ctx, n, 1 + j) for j in range(k)]
    t_other, t0, t5 = MLE.random(other, n, 1), MLE.random(ctx, 0, 2), MLE.random(ctx, 5, 3)
    before = [t.evaluation_slice().copy() for t in ts]
    five, zero = orc.from_int(field, 5), np.zeros(4, dtype=np.uint64)
    raw_p = np.frombuffer(p.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    fp, zp, pp = (x.ctypes.data_as(u64p) for x in (five, zero, raw_p))

    def arr(tables):
        a = (c.c_void_p * len(tables))(*[None if t is None else t._h.value for t in tables])
        return c.cast(a, c.POINTER(c.c_void_p)), a

    h = c.c_void_p()
    cm = lib.zk_mlbatch_commit
    good, _k1 = arr(ts)
    # NULL, another context, the shapes, the shift, the domain -- in this order; then the tables' sizes and contexts, k out of range
    assert cm(ctx._h, None, k, 1, fp, c.byref(h)) == BAD and cm(ctx._h, good, k, 1, None, c.byref(h)) == BAD and cm(ctx._h, good, k, 1, fp, None) == BAD
    hole, _k2 = arr([ts[0], None, ts[2]])
    assert cm(ctx._h, hole, k, 1, fp, c.byref(h)) == BAD
    assert cm(other._h, good, k, 0, zp, c.byref(h)) == MISMATCH
    mixed_ctx, _k3 = arr([ts[0], t_other, ts[2]])
    assert cm(ctx._h, mixed_ctx, k, 0, zp, c.byref(h)) == MISMATCH
    for b in (0, 9):
        assert cm(ctx._h, good, k, b, fp, c.byref(h)) == BAD, b
    zeros, _k4 = arr([t0, t0])
    assert cm(ctx._h, zeros, 2, 1, fp, c.byref(h)) == BAD                            # n = 0
    assert cm(ctx._h, good, k, 1, zp, c.byref(h)) == BAD and cm(ctx._h, good, k, 1, pp, c.byref(h)) == BAD
    mixed_n, _k5 = arr([ts[0], t5, ts[2]])
    assert cm(ctx._h, mixed_n, k, 1, fp, c.byref(h)) == BAD                          # tables of different n_vars
    many, _k6 = arr([ts[0]] * 257)
    assert cm(ctx._h, many, 0, 1, fp, c.byref(h)) == BAD and cm(ctx._h, many, 257, 1, fp, c.byref(h)) == BAD
    big = MLE.random(ctx, 21, 3)
    bigs, _k7 = arr([big, big])
    assert cm(ctx._h, bigs, 2, 8, fp, c.byref(h)) == NO_ROOT                         # BN254: two-adicity 28
    big.free()
    assert not h.value
    com = zk_amd.MultilinearBatchCommitment.commit(ts, 1, five)
    seed = np.arange(32, dtype=np.uint8)
    sp = seed.ctypes.data_as(u8p)
    m = 2
    buf = np.full(ref.proof_bytes(n, 1, 0, 8, k, m), 7, dtype=np.uint8)
    val = np.full((m, k, 4), 9, dtype=np.uint64)
    zs = [[0, 1, p - 1, 5, 6, 7], [3, 0, 1, p - 2, 8, 9]]
    points = np.ascontiguousarray(_points(field, zs))
    bad_points = points.copy()
    bad_points[1, 4] = raw_p
    bp, vp, zq, zbad = buf.ctypes.data_as(u8p), val.ctypes.data_as(u64p), points.ctypes.data_as(u64p), bad_points.ctypes.data_as(u64p)
    opn = lib.zk_mlbatch_open
    assert opn(ctx._h, com._h, None, m, 0, 8, sp, vp, bp) == BAD and opn(ctx._h, com._h, zq, m, 0, 8, None, vp, bp) == BAD
    assert opn(ctx._h, com._h, zq, m, 0, 8, sp, None, bp) == BAD and opn(ctx._h, None, zq, m, 0, 8, sp, vp, bp) == BAD
    assert opn(other._h, com._h, zq, 0, 0, 8, sp, vp, bp) == MISMATCH
    for f, nq, mm in ((n, 8, m), (n + 3, 8, m), (0, 0, m), (0, 1025, m), (0, 8, 0), (0, 8, 17)):
        assert opn(ctx._h, com._h, zq, mm, f, nq, sp, vp, bp) == BAD, (f, nq, mm)
    assert opn(ctx._h, com._h, zbad, m, 0, 8, sp, vp, bp) == BAD
    root_buf = np.zeros(32, dtype=np.uint8)
    assert lib.zk_mlbatch_root(other._h, com._h, root_buf.ctypes.data_as(u8p)) == MISMATCH
    cnt = c.c_uint32(77)
    assert lib.zk_mlbatch_n_tables(None, c.byref(cnt)) == BAD and lib.zk_mlbatch_n_vars(com._h, None) == BAD and cnt.value == 77
    # zk_mle_eq_sums_many
    sums = np.full((m, 2, 4), 9, dtype=np.uint64)
    sq = sums.ctypes.data_as(u64p)
    tails = np.ascontiguousarray(points[:, 1:])
    bad_tails = np.ascontiguousarray(bad_points[:, 1:])
    tq, tbad = tails.ctypes.data_as(u64p), bad_tails.ctypes.data_as(u64p)
    es = lib.zk_mle_eq_sums_many
    assert es(ctx._h, ts[0]._h, None, m, sq) == BAD and es(ctx._h, None, tq, m, sq) == BAD and es(ctx._h, ts[0]._h, tq, m, None) == BAD
    assert es(other._h, ts[0]._h, tq, m, sq) == MISMATCH and es(ctx._h, t0._h, tq, m, sq) == BAD
    assert es(ctx._h, ts[0]._h, tq, 0, sq) == BAD and es(ctx._h, ts[0]._h, tq, 17, sq) == BAD
    assert es(ctx._h, ts[0]._h, tbad, m, sq) == BAD                                  # a tail element is not reduced
    # zk_mle_lincomb
    out = MLE.random(ctx, n, 50)
    out_before = out.evaluation_slice().copy()
    out_other, out5 = MLE.alloc(other, n), MLE.alloc(ctx, 5)
    coeffs = np.ascontiguousarray(orc.from_ints(field, [2, p - 1, 0]))
    bad_coeffs = coeffs.copy()
    bad_coeffs[1] = raw_p
    cq, cbad = coeffs.ctypes.data_as(u64p), bad_coeffs.ctypes.data_as(u64p)
    lc = lib.zk_mle_lincomb
    assert lc(ctx._h, None, k, cq, out._h) == BAD and lc(ctx._h, good, k, None, out._h) == BAD and lc(ctx._h, good, k, cq, None) == BAD
    assert lc(ctx._h, hole, k, cq, out._h) == BAD and lc(ctx._h, good, 0, cq, out._h) == BAD and lc(ctx._h, many, 257, cq, out._h) == BAD
    assert lc(ctx._h, good, k, cq, out_other._h) == MISMATCH and lc(ctx._h, mixed_ctx, k, cq, out._h) == MISMATCH
    assert lc(ctx._h, good, k, cq, out5._h) == BAD and lc(ctx._h, mixed_n, k, cq, out._h) == BAD
    assert lc(ctx._h, good, k, cq, ts[1]._h) == BAD                                  # out aliases a source
    assert lc(ctx._h, good, k, cbad, out._h) == BAD
    # nothing was written by any of them
    assert (buf == 7).all() and (val == 9).all() and (sums == 9).all() and not root_buf.any() and np.array_equal(out.evaluation_slice(), out_before)
    assert opn(ctx._h, com._h, zq, m, 0, 8, sp, vp, bp) == 0
    tables = [orc.to_ints(field, s) for s in before]
    want_v, want = ref.prove(field, tables, 1, 0, 8, 5, seed.tobytes(), zs)
    assert buf.tobytes() == want and [orc.to_ints(field, row) for row in val] == want_v
    assert es(ctx._h, ts[0]._h, tq, m, sq) == 0
    assert [orc.to_ints(field, pair) for pair in sums] == ref.eq_sums_many(tables[0], [z[1:] for z in zs], p)
    assert lc(ctx._h, good, k, cq, out._h) == 0
    assert orc.to_ints(field, out.evaluation_slice()) == ref.lincomb(tables, [2, p - 1, 0], p)
    one_var = MLE.new(ctx, 1, orc.from_ints(field, [3, p - 1]))
    assert [orc.to_ints(field, x) for x in zk_amd.eq_sums_many(one_var, np.zeros((2, 0, 4), dtype=np.uint64))] == [[3, p - 1]] * 2   # m = 0: S_X = t[X]
    # the measurement hook gives a positive time on every path and leaves the handle's tables alone
    root = com.root()
    ms = c.c_double(-1.0)
    for path in (0, 1, 2, 3, 4):
        ms.value = -1.0
        assert lib.zk_bench_mlbatch(ctx._h, com._h, 2, path, 2, c.byref(ms)) == 0 and ms.value > 0, path
    assert zk_amd.bench_mlbatch(com, n_points=ref.POINTS_PER_PASS + 1, path=0, reps=1) > 0
    ms.value = -1.0
    bm = lib.zk_bench_mlbatch
    assert bm(ctx._h, com._h, 1, 5, 1, c.byref(ms)) == BAD and bm(ctx._h, com._h, 1, 0, 0, c.byref(ms)) == BAD and bm(ctx._h, com._h, 1, -1, 1, c.byref(ms)) == BAD
    assert bm(ctx._h, com._h, 0, 0, 1, c.byref(ms)) == BAD and bm(ctx._h, com._h, 17, 0, 1, c.byref(ms)) == BAD and bm(ctx._h, None, 1, 0, 1, c.byref(ms)) == BAD
    assert bm(other._h, com._h, 1, 0, 1, c.byref(ms)) == MISMATCH and ms.value == -1.0
    assert opn(ctx._h, com._h, zq, m, 0, 8, sp, vp, bp) == 0 and buf.tobytes() == want and com.root() == root   # the handle's copies are intact
    assert all(np.array_equal(t.evaluation_slice(), s) for t, s in zip(ts, before))
    com.free()
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_mlbatch.cpp over zk.hpp: openings, the verifier's verdicts, several openings of one commitment, lincomb, eq_sums_many,
    the errors"""
    exe = str(tmp_path / "test_mlbatch")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_mlbatch.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: mlbatch host tests passed" in r.stdout
