"""The definition of the fractional-sum argument (tests/fsum_ref.py) checked on its own, and the host verifier zk_fsum_verify_host against it
on the shared case list: every honest proof accepted by both with equal point and claims, every kind of change rejected by both with
equal verdicts, a cheating prover, a zero denominator, zk_fsum_proof_bytes, the argument table, the multiplicities and the lookup
composition in plain Python, the kernels' constants, the new exports and their Python signatures -- all without a GPU.  Everything is
bytes."""
import ctypes as c
import os
import re
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsum_ref as ref  # noqa: E402
import gprod_ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, BAD_FIELD = -20, -21
SYMBOLS = ("zk_mle_fraction_tree", "zk_fsum_proof_bytes", "zk_fsum_prove", "zk_fsum_verify_host", "zk_lookup_multiplicities", "zk_bench_fsum")
WRAPPERS = ("fraction_tree", "fractional_sum_prove", "fractional_sum_verify", "fsum_proof_bytes", "lookup_multiplicities", "bench_fsum",
            "lookup_prove", "lookup_verify")
UNTOUCHED = 0x0909090909090909


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _raw(v):
    """limbs of an integer as they are, reduced or not"""
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def _verify_raw(field, n, has_p, shift, seed, total, proof, proof_len=None, raw_shift=None, raw_total=None):
    """(status, ok, point, claims) of zk_fsum_verify_host on raw buffers; shift (None = NULL), total = (N, D): canonical ints; point and
    claims as ints when the proof was accepted, else whether the buffers were left alone"""
    ok = c.c_int32(-7)
    sv = raw_shift if raw_shift is not None else (None if shift is None else orc.from_int(field, shift))
    tv = np.ascontiguousarray(raw_total if raw_total is not None else orc.from_ints(field, list(total)))
    point, claims = np.full((41, 4), UNTOUCHED, dtype=np.uint64), np.full(8, UNTOUCHED, dtype=np.uint64)
    sd, pf = _u8(seed), _u8(proof)
    rc = _lib.lib.zk_fsum_verify_host(field, n, int(has_p), None if sv is None else sv.ctypes.data_as(_lib.u64p), sd.ctypes.data_as(_lib.u8p),
                                      tv.ctypes.data_as(_lib.u64p), pf.ctypes.data_as(_lib.u8p), len(proof) if proof_len is None else proof_len,
                                      point.ctypes.data_as(_lib.u64p), claims.ctypes.data_as(_lib.u64p), c.byref(ok))
    if rc == 0 and ok.value == 1:
        assert (point[n:] == UNTOUCHED).all()
        return rc, 1, orc.to_ints(field, point[:n]), tuple(orc.to_ints(field, claims.reshape(2, 4)))
    return rc, ok.value, bool((point == UNTOUCHED).all()), bool((claims == UNTOUCHED).all())


def _both(field, n, has_p, shift, seed, total, proof):
    """the verdict of the library and of the definition, which must be the same (with equal point and claims on acceptance)"""
    rc, ok, point, claims = _verify_raw(field, n, has_p, shift, seed, total, proof)
    want = ref.verify(field, n, has_p, seed, total, proof, shift)
    assert rc == 0 and ok == int(want is not None), (n, rc, ok, want)
    if want is None:
        assert point is True and claims is True   # nothing was written
        return None
    assert (point, claims) == (list(want[0]), want[1])
    return want


def _put(proof, at, value):
    return proof[:at] + int(value).to_bytes(32, "big") + proof[at + 32:]


@pytest.fixture(scope="module")
def proofs():
    """{case: (field, q, p_tab, shift, seed, (N, D), proof, point, claims)} for the shared case list from the definition, computed once"""
    out = {}
    for case in ref.CASES:
        field, q, p_tab, shift, seed = ref.case_inputs(case, worst_case_values)
        out[case] = (field, q, p_tab, shift, seed) + ref.prove(field, q, seed, p_tab, shift)
    return out


def _honest(proofs):
    return {case: v for case, v in proofs.items() if not case[2]}


def test_exports_signatures_and_makefile():
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(_lib.lib, name), name
        assert name in _lib._sig and name in _lib.declared_symbols(), name
        assert re.search(r"\bint32_t %s\(" % name, header), name
    for name in WRAPPERS:
        assert name in zk_amd.api.__all__ and hasattr(zk_amd, name), name
    make = open(os.path.join(ROOT, "zk_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS := .*\bfsum\.o\b", make, flags=re.M)
    assert 'env_u64("ZK_FSUM_TREE_FUSE"' in open(os.path.join(ROOT, "zk_amd", "csrc", "fsum.hip")).read()
    assert "ZK_FSUM_TREE_FUSE" in header


def test_case_lists_and_kernel_constants():
    assert sorted(cs[0] for cs in ref.CASES if not cs[2]) == sorted(list(range(1, 9)) * 2)
    assert {cs[2] for cs in ref.CASES} == {"", "cancel"}
    assert {ref.case_field(cs) for cs in ref.CASES} == {0, 1, 2}
    assert {ref.case_shift_kind(cs) for cs in ref.CASES} == set(ref.SHIFT_KINDS) and len(ref.SHIFT_KINDS) == 5
    for n in range(1, 9):   # every size with p given and with p = None
        assert {ref.case_has_p(cs) for cs in ref.CASES if cs[0] == n and not cs[2]} == {True, False}
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "fsum_kernels.cuh")).read()
    common = open(os.path.join(ROOT, "zk_amd", "csrc", "common.cuh")).read()
    core = open(os.path.join(ROOT, "zk_amd", "csrc", "host_core.hpp")).read()
    assert ref.THREADS == int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    assert ref.LDS_VARS == int(re.search(r"constexpr uint32_t kFtreeLdsVars = (\d+);", src).group(1))
    assert ref.FUSE_MAX == int(re.search(r"constexpr uint32_t kFtreeMaxFuse = (\d+);", src).group(1))
    assert ref.FUSE_DEFAULT == int(re.search(r"constexpr uint32_t kFtreeFuseDefault = (\d+);", src).group(1))
    mt, mw = re.search(r"constexpr uint32_t kMultMaxTableVars = (\d+), kMultMaxWitnessVars = (\d+);", src).groups()
    assert (ref.MULT_MAX_TABLE_VARS, ref.MULT_MAX_WITNESS_VARS) == (int(mt), int(mw))
    assert ref.MAX_BLOCKS_STREAM == int(re.search(r"constexpr uint32_t kMaxGridStream = (\d+);", core).group(1))
    assert ref.MAX_BLOCKS == int(re.search(r"constexpr uint32_t kMaxGrid = (\d+);", core).group(1))
    assert ref.MAX_VARS == int(re.search(r"constexpr uint64_t kMaxVars = (\d+);", core).group(1))
    L = ref.LDS_VARS
    # both halves of a level of 2^L elements of each heap fit the static LDS of one workgroup (64 KiB) beside each other
    assert 2 * (32 << (L - 1)) <= 64 * 1024
    assert (1 << L) % ref.THREADS == 0 and ref.THREADS % 64 == 0
    assert ref.launches(L) == [] and ref.launches(1) == [] and ref.FUSE_MAX == 2
    assert [ref.launches(L + k) for k in (1, 2, 3, 4)] == [[(1, L)], [(2, L)], [(2, L + 1), (1, L)], [(2, L + 2), (2, L)]]
    assert ref.launches(L + 3, 1) == [(1, L + 2), (1, L + 1), (1, L)]
    extra = ref.GPU_EXTRA_CASES   # every arity of the fused kernel, then two launches; both kinds of p; all three fields; nothing above 2^14
    assert [cs[0] - L for cs in extra] == [1, 2, 3, 4] and {ref.case_has_p(cs) for cs in extra} == {True, False}
    assert {ref.case_field(cs) for cs in extra} == {0, 1, 2} and max(cs[0] for cs in extra) <= 14
    assert ref.TREE_VARS == tuple(range(1, L + 3))
    assert ref.SECOND_TRIP_VARS == {1: 24, 2: 25} and ref.trips(23, 1) == 1 and ref.trips(24, 1) == 2
    assert ref.MULT_SECOND_TRIP_VARS == 20 and (1 << 19) == ref.MAX_BLOCKS * ref.THREADS


def test_the_tree_is_the_sum_of_fractions(proofs):
    for case, (field, q, p_tab, shift, seed, total, proof, point, claims) in proofs.items():
        p = orc.modulus(field)
        n = case[0]
        P, Q = ref.tree(q, p_tab, shift, p)
        heap_p, heap_q = ref.fraction_tree(q, p_tab, shift, p)
        assert total == (P[0][0], Q[0][0]) == (heap_p[1], heap_q[1]) and heap_p[0] == 0 and heap_q[0] == 1
        assert len(heap_p) == len(heap_q) == 1 << n
        assert heap_q == gprod_ref.product_tree(q, shift, p)   # the Q heap is the grand product's tree
        for j in range(n):
            assert heap_p[1 << j:2 << j] == P[j] and heap_q[1 << j:2 << j] == Q[j]
        if case[2] == "cancel":   # nothing is inverted: a zero denominator is D = 0, not an error
            assert total[1] == 0 and any((x + (shift or 0)) % p == 0 for x in q)
            continue
        assert total[1] != 0 and total[0] * pow(total[1], p - 2, p) % p == ref.fractional_sum(q, p_tab, shift, p)
        for j in (0, n // 2):   # a node is the sum of the fractions of the leaves that agree with it in the low j index bits
            for i in (0, (1 << j) - 1):
                sub_q = [q[k] for k in range(i, 1 << n, 1 << j)]
                sub_p = None if p_tab is None else [p_tab[k] for k in range(i, 1 << n, 1 << j)]
                assert P[j][i] * pow(Q[j][i], p - 2, p) % p == ref.fractional_sum(sub_q, sub_p, shift, p)


def test_completeness_and_proof_bytes(proofs):
    for case, (field, q, p_tab, shift, seed, total, proof, point, claims) in _honest(proofs).items():
        n = case[0]
        p = orc.modulus(field)
        has_p = p_tab is not None
        got = ref.verify(field, n, has_p, seed, total, proof, shift)
        assert got == (point, claims) and len(point) == n, case
        assert claims == (ref.evaluate(p_tab if has_p else [1] * len(q), point, p), ref.evaluate(q, point, p)), case   # the claims left are true
        assert has_p or claims[0] == 1
        assert _both(field, n, has_p, shift, seed, total, proof) is not None, case
        assert len(proof) == ref.proof_bytes(n) == zk_amd.fsum_proof_bytes(n) == 64 * n * (n + 1), case
        out = zk_amd.fractional_sum_verify(field, n, has_p, seed, orc.from_ints(field, list(total)), proof, None if shift is None else orc.from_int(field, shift))
        assert out is not None and orc.to_ints(field, out[0]) == point and tuple(orc.to_ints(field, out[1])) == claims


def test_null_and_zero_shift_give_the_same_bytes(proofs):
    seen = set()
    for case, (field, q, p_tab, shift, seed, total, proof, point, claims) in _honest(proofs).items():
        if shift in (None, 0):
            seen.add(shift)
            for other in (None, 0):
                assert ref.prove(field, q, seed, p_tab, other) == (total, proof, point, claims)
                assert _both(field, case[0], p_tab is not None, other, seed, total, proof) == (point, claims)
    assert seen == {None, 0}


def test_every_change_is_rejected_by_both(proofs):
    for case, (field, q, p_tab, shift, seed, total, proof, point, claims) in _honest(proofs).items():
        n = case[0]
        p = orc.modulus(field)
        has_p = p_tab is not None
        N, D = total
        for bad_total in (((N + 1) % p, D), (N, (D + 1) % p), (N, 0)):
            assert _both(field, n, has_p, shift, seed, bad_total, proof) is None, case
        # another seed, shift or has_p is another transcript: from n = 2 on layer 1's first round check fails; at n = 1 there is no later
        # check (layer 0's two equations hold) and what changes is the point and the claims that are handed out -- unless has_p = 0 is
        # claimed for a proof with p != ones, which the check cP_n = 1 rejects at every n
        others = (_both(field, n, has_p, shift, bytes([seed[0] ^ 1]) + seed[1:], total, proof),
                  _both(field, n, has_p, ((shift or 0) + 1) % p, seed, total, proof), _both(field, n, not has_p, shift, seed, total, proof))
        for k, got in enumerate(others):
            if n >= 2 or (k == 2 and has_p):
                assert got is None, (case, k)
            else:
                assert got is not None and got[0] != point, (case, k)
        if n >= 3:   # one element changed in each section
            offsets = ref.section_offsets(n)
            assert set(offsets) == {"l0_p0", "l0_p1", "l0_q0", "l0_q1", "round_first", "round_last", "p0", "p1", "q0", "q1"}
            assert offsets["q1"] == len(proof) - 32
            for name, at in offsets.items():
                bad = bytearray(proof)
                bad[at + 31] ^= 1
                assert _both(field, n, has_p, shift, seed, total, bytes(bad)) is None, (case, name)
                assert _both(field, n, has_p, shift, seed, total, _put(proof, at, p)) is None, (case, name)   # an element >= p
        else:
            for at in range(0, len(proof), 32):
                bad = bytearray(proof)
                bad[at + 31] ^= 1
                got = _both(field, n, has_p, shift, seed, total, bytes(bad))
                # the last layer's four values feed no later equation but the claims: a change there that keeps the layer's equation
                # cannot happen with one element, so every change is rejected
                assert got is None, (case, at)
        for other in (proof[:-1], proof + b"\0", proof[:-32], proof + proof[-32:]):
            assert ref.verify(field, n, has_p, seed, total, other, shift) is None
            assert _verify_raw(field, n, has_p, shift, seed, total, other) == (BAD, -7, True, True)
        for m in (n - 1, n + 1):
            if m >= 1:
                assert ref.verify(field, m, has_p, seed, total, proof, shift) is None
                assert _verify_raw(field, m, has_p, shift, seed, total, proof) == (BAD, -7, True, True)
        padded = (proof + bytes(ref.proof_bytes(n + 1)))[:ref.proof_bytes(n + 1)]
        assert _both(field, n + 1, has_p, shift, seed, total, padded) is None, case


def test_a_proof_made_with_another_p_is_rejected_without_p(proofs):
    """has_p = 0 promises p = ones: a prover that runs the argument with another p (the transcript says has_p = 0) passes every sumcheck,
    and is rejected by the check cP_n = 1"""
    for case, (field, q, p_tab, shift, seed, total, proof, point, claims) in _honest(proofs).items():
        if p_tab is not None:
            continue
        n = case[0]
        p = orc.modulus(field)
        other_p = [1] * len(q)
        other_p[-1] = 2
        levels = ref.tree(q, other_p, shift, p)
        total2, proof2, point2, claims2 = ref.prove(field, q, seed, None, shift, levels=levels)   # levels of p = other_p, transcript of p = None
        assert claims2[0] != 1 and claims2[0] == ref.evaluate(other_p, point2, p)
        assert _both(field, n, False, shift, seed, total2, proof2) is None, case


def test_a_cheating_prover_is_rejected(proofs):
    """the sumchecks are run on trees with one inner node changed, in P or in Q (so the claimed sum, or a layer's link, is false):
    deterministic under the fixed seeds, and rejected by both"""
    for case in [cs for cs in ref.CASES if cs[0] >= 2 and not cs[2]]:
        field, q, p_tab, shift, seed = proofs[case][:5]
        n = case[0]
        p = orc.modulus(field)
        for j in sorted({0, n // 2, n - 1}):
            for which in (0, 1):
                levels = tuple([list(level) for level in heap] for heap in ref.tree(q, p_tab, shift, p))
                levels[which][j][(1 << j) - 1] = (levels[which][j][(1 << j) - 1] + 1) % p
                total, proof, point, claims = ref.prove(field, q, seed, p_tab, shift, levels=levels)
                assert _both(field, n, p_tab is not None, shift, seed, total, proof) is None, (case, j, which)


def test_a_zero_denominator_is_rejected(proofs):
    case = next(cs for cs in ref.CASES if cs[2] == "cancel")
    field, q, p_tab, shift, seed, total, proof, point, claims = proofs[case]
    assert total[1] == 0 and ref.verify(field, case[0], p_tab is not None, seed, total, proof, shift) is None
    assert _both(field, case[0], p_tab is not None, shift, seed, total, proof) is None


def test_argument_table(proofs):
    case = (4, 0, "")
    field, q, p_tab, shift, seed, total, proof, point, claims = proofs[case]
    n = 4
    p = orc.modulus(field)
    u64p, u8p = _lib.u64p, _lib.u8p
    assert _verify_raw(field, n, True, shift, seed, total, proof)[:2] == (0, 1)
    sd, pf, tv = _u8(seed), _u8(proof), np.ascontiguousarray(orc.from_ints(field, list(total)))
    pt, cl, ok = np.full((n, 4), UNTOUCHED, dtype=np.uint64), np.full(8, UNTOUCHED, dtype=np.uint64), c.c_int32(-7)
    args = [field, n, 1, None, sd.ctypes.data_as(u8p), tv.ctypes.data_as(u64p), pf.ctypes.data_as(u8p), len(proof), pt.ctypes.data_as(u64p),
            cl.ctypes.data_as(u64p), c.byref(ok)]
    for i in (4, 5, 6, 8, 9, 10):   # every pointer but the shift
        bad = list(args)
        bad[i] = None
        assert _lib.lib.zk_fsum_verify_host(*bad) == BAD, i
    # a NULL with an unknown field: the NULL is reported; an unknown field before a bad n
    assert _lib.lib.zk_fsum_verify_host(7, n, 1, None, None, *args[5:]) == BAD
    assert _lib.lib.zk_fsum_verify_host(7, 0, *args[2:]) == BAD_FIELD
    assert (pt == UNTOUCHED).all() and (cl == UNTOUCHED).all() and ok.value == -7
    for bad_n in (0, 41):
        assert _verify_raw(field, bad_n, True, shift, seed, total, proof) == (BAD, -7, True, True)
    assert _verify_raw(field, n, True, shift, seed, total, proof, raw_shift=_raw(p)) == (BAD, -7, True, True)
    for raw in (np.stack([_raw(p), _raw(total[1])]), np.stack([_raw(1), _raw(p)]), np.stack([_raw(1), _raw((1 << 256) - 1)])):
        assert _verify_raw(field, n, True, shift, seed, total, proof, raw_total=raw) == (BAD, -7, True, True)
    assert _verify_raw(field, n, True, shift, seed, total, proof, proof_len=len(proof) - 32) == (BAD, -7, True, True)
    out = c.c_uint64(5)
    for bad_n in (0, 41, 1 << 31):
        assert _lib.lib.zk_fsum_proof_bytes(bad_n, c.byref(out)) == BAD and out.value == 5
    assert _lib.lib.zk_fsum_proof_bytes(4, None) == BAD
    assert _lib.lib.zk_fsum_proof_bytes(40, c.byref(out)) == 0 and out.value == 64 * 40 * 41
    # the device calls refuse a NULL context before anything else, without a GPU
    h = c.c_void_p()
    cnt = c.c_uint64(3)
    assert _lib.lib.zk_mle_fraction_tree(None, None, None, None, c.byref(h), c.byref(h)) == BAD and not h.value
    assert _lib.lib.zk_lookup_multiplicities(None, None, None, c.byref(h), c.byref(cnt), c.byref(cnt), c.byref(cnt)) == BAD and cnt.value == 3
    ms = c.c_double(-1.0)
    assert _lib.lib.zk_bench_fsum(None, None, 0, 1, c.byref(ms)) == BAD and ms.value == -1.0


def test_multiplicities_definition():
    table = [5, 9, 5, 7, 9, 5, 11, 0]
    witness = [9, 5, 5, 3, 0, 9, 12, 5]
    assert ref.multiplicities(table, witness) == ([3, 2, 0, 0, 0, 0, 0, 1], 2, 3, 3)
    assert ref.multiplicities(table, table) == ([3, 2, 0, 1, 0, 0, 1, 1], 0, ref.NONE_MISSING, 3)
    assert ref.multiplicities([4], [4, 4]) == ([2], 0, (1 << 64) - 1, 0) and ref.multiplicities([4], [5]) == ([0], 1, 0, 0)
    # the identity the lookup rests on: sum_i 1 / (w_i + a) = sum_j m_j / (t_j + a) when nothing is missing
    p = orc.modulus(0)
    m = ref.multiplicities(table, [x for x in witness if x in table])[0]
    a = 123456789
    assert ref.fractional_sum([x for x in witness if x in table], None, a, p) == ref.fractional_sum(table, m, a, p)


def test_lookup_composition_in_plain_python():
    field = 0
    p = orc.modulus(field)
    import random
    rng = random.Random(5)
    table = rng.sample(range(1, 1 << 30), 8)
    witness = [rng.choice(table) for _ in range(16)]
    seed, alpha = bytes(range(32)), rng.randrange(p)
    m, proof = ref.lookup_prove(field, witness, table, alpha, seed)
    assert m == ref.multiplicities(table, witness)[0] and sum(m) == len(witness)
    got = ref.lookup_verify(field, 4, 3, alpha, seed, proof)
    assert got is not None
    (r_f, f_claim), (r_t, t_claim, m_claim) = got
    assert (f_claim, t_claim, m_claim) == (ref.evaluate(witness, r_f, p), ref.evaluate(table, r_t, p), ref.evaluate(m, r_t, p))
    assert ref.lookup_seeds(seed)[0] != ref.lookup_seeds(seed)[1]
    # the host verifier agrees, through the public Python composition
    lim = lambda t: orc.from_ints(field, list(t))
    got_lib = zk_amd.lookup_verify(field, 4, 3, orc.from_int(field, alpha), seed, (lim(proof[0]), proof[1], lim(proof[2]), proof[3]))
    assert got_lib is not None and orc.to_ints(field, got_lib[0][0]) == r_f and orc.to_int(field, got_lib[1][2]) == m_claim
    # one witness entry changed to an absent value
    bad = list(witness)
    bad[5] = 1 << 31
    with pytest.raises(ValueError, match=r"witness entry 5 \(first_missing\)"):
        ref.lookup_prove(field, bad, table, alpha, seed)
    # m tampered by +-1: each side is a true statement about its tables, and the two sums differ
    sf, st = ref.lookup_seeds(seed)
    hit = next(j for j, v in enumerate(m) if v)
    for delta in (1, -1):
        forged = list(m)
        forged[hit] = (forged[hit] + delta) % p
        tot_t, proof_t, _, _ = ref.prove(field, table, st, forged, alpha)
        assert ref.verify(field, 3, True, st, tot_t, proof_t, alpha) is not None
        forged_proof = (proof[0], proof[1], tot_t, proof_t)
        assert ref.lookup_verify(field, 4, 3, alpha, seed, forged_proof) is None
        assert zk_amd.lookup_verify(field, 4, 3, orc.from_int(field, alpha), seed, (lim(proof[0]), proof[1], lim(tot_t), proof_t)) is None
    # the two proofs on each other's seeds, or with another alpha, are rejected
    assert ref.lookup_verify(field, 4, 3, (alpha + 1) % p, seed, proof) is None
    assert ref.lookup_verify(field, 4, 3, alpha, bytes(32), proof) is None
