"""The definition of the multilinear polynomial commitment (tests/mlpcs_ref.py) checked on its own, and the host verifier
zk_mlpcs_verify_host against it on the shared case list: every honest proof accepted by both, every kind of change rejected by both with
equal verdicts, two cheating provers, zk_mlpcs_proof_bytes, the argument table, the round kernel's constants, the new exports and their
Python signatures -- all without a GPU.  Everything is bytes."""
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
import cmle_ref  # noqa: E402
import fri_ref  # noqa: E402
import mlpcs_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ROOT, BAD, BAD_FIELD = -7, -20, -21
SYMBOLS = ("zk_mlpcs_commit", "zk_mlpcs_free", "zk_mlpcs_n_vars", "zk_mlpcs_root", "zk_mlpcs_proof_bytes", "zk_mlpcs_open",
           "zk_mlpcs_verify_host", "zk_mle_eq_sums", "zk_bench_mlpcs_round")
WRAPPERS = ("MultilinearCommitment", "mlpcs_verify", "mlpcs_proof_bytes", "eq_sums", "bench_mlpcs_round")


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _raw(v):
    """limbs of an integer as they are, reduced or not"""
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def _verify_raw(field, case, shift, seed, root, z, v, proof, proof_len=None, raw_point=None, raw_value=None, raw_shift=None, call_field=None):
    """(status, ok) of zk_mlpcs_verify_host on raw buffers; shift, z, v: canonical ints"""
    n, b, f, q = case
    ok = c.c_int32(-7)
    sv = orc.from_int(field, shift) if raw_shift is None else raw_shift
    zv = np.ascontiguousarray(orc.from_ints(field, list(z))) if raw_point is None else raw_point
    vv = orc.from_int(field, v) if raw_value is None else raw_value
    sd, rt, pv = _u8(seed), _u8(root), _u8(proof)
    rc = _lib.lib.zk_mlpcs_verify_host(field if call_field is None else call_field, n, b, f, q, sv.ctypes.data_as(_lib.u64p), sd.ctypes.data_as(_lib.u8p), rt.ctypes.data_as(_lib.u8p),
                                       zv.ctypes.data_as(_lib.u64p), vv.ctypes.data_as(_lib.u64p), pv.ctypes.data_as(_lib.u8p),
                                       len(proof) if proof_len is None else proof_len, c.byref(ok))
    return rc, ok.value


def _both(field, case, shift, seed, root, z, v, proof):
    """the verdict of the library and of the definition, which must be the same"""
    n, b, f, q = case
    rc, ok = _verify_raw(field, case, shift, seed, root, z, v, proof)
    want = ref.verify(field, n, b, f, q, shift, seed, root, z, v, proof)
    assert rc == 0 and ok == int(want), (case, rc, ok, want)
    return want


def _put(proof, at, value):
    return proof[:at] + int(value).to_bytes(32, "big") + proof[at + 32:]


@pytest.fixture(scope="module")
def proofs():
    """{case: (field, table, shift, seed, z, root, v, the definition's proof)} for the shared case list, computed once"""
    out = {}
    for case in ref.CASES:
        n, b, f, q = case
        field = ref.case_field(case)
        table, shift, seed, z = ref.case_inputs(field, case, worst_case_values)
        committed = ref.commit(field, table, b, shift)
        v, proof = ref.prove(field, table, b, f, q, shift, seed, z, committed=committed)
        out[case] = (field, table, shift, seed, z, ref.merkle_ref.root(committed[2]), v, proof)
    return out


def test_exports_signatures_and_abi_version():
    assert _lib.lib.zk_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(_lib.lib, name), name
        assert name in _lib._sig and name in _lib.declared_symbols(), name
        assert re.search(r"\bint32_t %s\(" % name, header), name
    for name in WRAPPERS:
        assert name in zk_amd.api.__all__ and hasattr(zk_amd, name), name
    make = open(os.path.join(ROOT, "zk_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS := .*\bmlpcs\.o\b", make, flags=re.M)
    assert 'env_u64("ZK_MLPCS_ROUND"' in open(os.path.join(ROOT, "zk_amd", "csrc", "mlpcs.hip")).read()


def test_case_lists_and_kernel_constants():
    want = {(n, b, f, q) for n in range(1, 9) for b in (1, 2) for f in (0, 1, 2) for q in (1, 8) if f < n}
    assert set(ref.CASES) == want and len(ref.CASES) == len(want)
    assert {ref.case_field(cs) for cs in ref.CASES} == {0, 1, 2}
    assert set(ref.GPU_CASES) == {cs for cs in ref.CASES if cs[3] == 8} | {(11, 1, 2, 8), (12, 2, 0, 8), (13, 1, 1, 1)}
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "mlpcs_kernels.cuh")).read()
    common = open(os.path.join(ROOT, "zk_amd", "csrc", "common.cuh")).read()
    core = open(os.path.join(ROOT, "zk_amd", "csrc", "host_core.hpp")).read()
    assert ref.THREADS == int(re.search(r"constexpr int kBlock = (\d+);", common).group(1)) and ref.WAVE == 64
    assert ref.LO_BITS == int(re.search(r"constexpr uint32_t kMlLoBits = (\d+);", src).group(1))
    assert ref.RUN_MIN_BITS == int(re.search(r"constexpr uint32_t kMlRunMinBits = (\d+);", src).group(1))
    assert ref.MAX_BLOCKS == int(re.search(r"constexpr uint32_t kMaxGrid = (\d+);", core).group(1))
    assert ref.RUN_MIN_BITS <= ref.LO_BITS and 1 << ref.RUN_MIN_BITS == ref.WAVE   # a launch below the run kernel needs no Hi table
    L = ref.LO_BITS
    # no Hi table, one entry, two; one workgroup's four waves busy, then two workgroups
    assert [ref.hi_entries(n) for n in (L, L + 1, L + 2)] == [0, 1, 2]
    assert ref.RUNS_TARGET_LOG == int(re.search(r"constexpr uint32_t kMlRunsTargetLog = (\d+);", src).group(1))
    assert [(ref.runs(n), ref.blocks(n)) for n in (L, L + 1)] == [(4, 1), (8, 2)]
    assert ref.blocks(6) == 1 and ref.runs(7) == 1 and (ref.run_bits(15), ref.blocks(15)) == (6, 64)
    # the run length grows from 64 to 2^L elements between m = 17 and m = 20
    assert [ref.run_bits(n) for n in (18, 19, 20, 21, 22)] == [6, 7, 8, 9, 9] and {19, 20, 21} <= set(ref.ORACLE_SUMS_VARS)
    assert all(ref.RUN_MIN_BITS <= ref.run_bits(n) <= min(n - 1, L) for n in range(ref.RUN_MIN_BITS + 1, 41))
    # the capped grid: 2048 workgroups x 4 waves take one run each up to 2^13 runs; a second trip from m = L + 14 on
    assert ref.SECOND_TRIP_VARS == L + 15 == 24 and ref.trips(23) == 1 and ref.trips(24) == 2 and ref.blocks(24) == ref.MAX_BLOCKS
    assert ref.SECOND_TRIP_VARS in ref.ORACLE_SUMS_VARS
    assert {1, 2, 6, 7, 8, L, L + 1, L + 2, L + 3, L + 4} <= set(ref.EQ_SUMS_VARS)
    # the extra GPU cases pass through every regime: rounds with a Hi table (m > L), with L = m < LO_BITS in the run kernel, and below it
    for n, b, f, q in ref.GPU_EXTRA_CASES:
        ms = {n - 1 - r for r in range(n - f)}
        assert max(ms) > L and any(ref.RUN_MIN_BITS <= m < L for m in ms) and any(m < ref.RUN_MIN_BITS for m in ms)
        assert 12 <= n + b <= 14


def test_the_two_device_sums_give_the_round_polynomial():
    """h(0), h(1), h(2) from S_0, S_1 (mlpcs_ref.sums_to_round) equal the two-table round sums of (T, E c): the route does not matter"""
    for field in range(3):
        p = fri_ref.modulus(field)
        for n in (1, 2, 5):
            table, tail = ref.eq_sums_case(field, n, worst_case_values)
            for z0 in ref.point_entries(p, __import__("random").Random(n)):
                e = ref.eq_table([z0] + tail, p)
                s0, s1 = ref.eq_sums(table, tail, p)
                assert ref.sums_to_round(s0, s1, 7, z0, p) == [7 * x % p for x in ref.round_sums(table, e, p)]
                assert ref.evaluate(table, [z0] + tail, p) == ((1 - z0) * s0 + z0 * s1) % p


def test_folding_the_codeword_is_folding_the_table():
    """after every round the folded layer is the LDE of the coefficient form of the folded table over the squared coset"""
    field, n, b, s = 0, 5, 1, 5
    p = fri_ref.modulus(field)
    table = ref.case_table(p, field, n, worst_case_values)
    layer = ref.commit(field, table, b, s)[0]
    for r, beta in enumerate((3, p - 1, 0, 1, 12345)):
        table, layer = ref.partial_evaluate0(table, beta, p), fri_ref.fold(field, layer, s, beta, 1)
        s = s * s % p
        co = cmle_ref.interpolate_fast(table, p)[1] if len(table) > 1 else list(table)
        assert layer == fri_ref.lde(field, co, n - r - 1 + b, s), r
    assert len(set(layer)) == 1 and layer[0] == table[0]


def test_completeness_and_proof_bytes(proofs):
    for case, (field, table, shift, seed, z, root, v, proof) in proofs.items():
        n, b, f, q = case
        p = fri_ref.modulus(field)
        assert v == cmle_ref.evaluate_slice(n, cmle_ref.interpolate_fast(table, p)[1], z, p)   # t(z) by the coefficient form too
        assert _both(field, case, shift, seed, root, z, v, proof) is True, case
        assert len(proof) == ref.proof_bytes(*case) == zk_amd.mlpcs_proof_bytes(*case), case
        assert zk_amd.mlpcs_verify(field, root, orc.from_ints(field, z), orc.from_int(field, v), proof, b, f, q, orc.from_int(field, shift), seed)
    kinds = {x for (field, table, shift, seed, z, *_r) in proofs.values() for x in z}
    assert {0, 1} <= kinds and any(x == fri_ref.modulus(0) - 1 for x in kinds)


def test_every_change_is_rejected_by_both(proofs):
    for case, (field, table, shift, seed, z, root, v, proof) in proofs.items():
        n, b, f, q = case
        p = fri_ref.modulus(field)
        assert _both(field, case, shift, seed, root, z, (v + 1) % p, proof) is False, case
        for j in range(n):
            z2 = list(z)
            z2[j] = (z[j] + 1) % p
            assert _both(field, case, shift, seed, root, z2, v, proof) is False, (case, j)
        seed2 = bytes([seed[0] ^ 1]) + seed[1:]
        assert _both(field, case, shift, seed2, root, z, v, proof) is False, case
        # one byte flipped in each section: an h, a root, a final coefficient, a row element, a path digest
        for name, at in ref.section_offsets(*case).items():
            if at is None or at >= len(proof):
                continue
            bad = bytearray(proof)
            bad[at + 31] ^= 1
            assert _both(field, case, shift, seed, root, z, v, bytes(bad)) is False, (case, name)
            assert _both(field, case, shift, seed, root, z, v, _put(proof, at, p)) is False, (case, name)   # an element >= p (a digest: another one)
        # a truncated and a lengthened proof: the definition rejects, the library refuses the length
        for other in (proof[:-1], proof + b"\0", proof[:-32], proof + proof[-32:]):
            assert not ref.verify(field, n, b, f, q, shift, seed, root, z, v, other)
            assert _verify_raw(field, case, shift, seed, root, z, v, other) == (BAD, -7)


def test_other_parameters_are_rejected(proofs):
    """the same bytes under another n, b, f or Q: mostly another length (refused), otherwise rejected by both"""
    for case in [cs for cs in ref.CASES if cs[0] in (3, 6)]:
        field, table, shift, seed, z, root, v, proof = proofs[case]
        n, b, f, q = case
        for other in ((n + 1, b, f, q), (n - 1, b, f, q), (n, b + 1, f, q), (n, b, f + 1, q), (n, b, max(f - 1, 0), q), (n, b, f, q + 1)):
            if other == case or other[2] >= other[0]:
                continue
            zo = (list(z) + [0])[:other[0]]
            if ref.proof_bytes(*other) != len(proof):
                assert _verify_raw(field, other, shift, seed, root, zo, v, proof) == (BAD, -7), (case, other)
                assert not ref.verify(field, *other, shift, seed, root, zo, v, proof)
            else:
                assert _both(field, other, shift, seed, root, zo, v, proof) is False, (case, other)
    # two shapes with equal lengths exist in the list (so the transcript's parameters, not the length alone, are what rejects them)
    field, table, shift, seed, z, root, v, proof = proofs[(4, 1, 1, 8)]
    same = [(n, b, f, 8) for n in range(1, 9) for b in (1, 2) for f in range(n) if ref.proof_bytes(n, b, f, 8) == len(proof) and (n, b, f) != (4, 1, 1)]
    for other in same:
        assert _both(field, other, shift, seed, root, (list(z) + [0] * 8)[:other[0]], v, proof) is False, other


def test_two_cheating_provers(proofs):
    """a prover that commits t but runs the sumcheck on a t' that differs in one entry, and one whose layer 0 is the LDE of 2^n + 1
    coefficients: the verdicts are deterministic under the fixed seeds, and both reject"""
    for case in [cs for cs in ref.CASES if cs[3] == 8 and cs[0] >= 2]:
        field, table, shift, seed, z, root, v, proof = proofs[case]
        n, b, f, q = case
        p = fri_ref.modulus(field)
        # the changed entry: where eq(., z) does not vanish in the variables the final polynomial keeps (z_j = 1 -> bit 1, else bit 0), or
        # t'(z) = t(z) and the claim would be true; the folded variables meet random betas
        at = sum((1 if (z[j] == 1 or (j < n - f and j % 2)) else 0) << (n - 1 - j) for j in range(n))
        other = list(table)
        other[at] = (other[at] + 1) % p
        v2, proof2 = ref.prove(field, table, b, f, q, shift, seed, z, sumcheck_table=other)
        assert v2 == ref.evaluate(other, z, p)
        assert _both(field, case, shift, seed, root, z, v2, proof2) is False, case
        coeffs = cmle_ref.interpolate_fast(table, p)[1] + [1 + case[0]]   # one coefficient past the bound
        layer0 = fri_ref.lde(field, coeffs, n + b, shift)
        committed = ref.commit(field, table, b, shift, layer0=layer0)
        v3, proof3 = ref.prove(field, table, b, f, q, shift, seed, z, committed=committed)
        assert v3 == v
        assert _both(field, case, shift, seed, ref.merkle_ref.root(committed[2]), z, v3, proof3) is False, case


def test_argument_table(proofs):
    case = (4, 1, 1, 8)
    field, table, shift, seed, z, root, v, proof = proofs[case]
    p = fri_ref.modulus(field)
    assert _verify_raw(field, case, shift, seed, root, z, v, proof) == (0, 1)
    assert _verify_raw(field, case, shift, seed, root, z, v, proof, call_field=7) == (BAD_FIELD, -7)
    for bad in ((0, 1, 0, 8), (4, 0, 1, 8), (4, 9, 1, 8), (4, 1, 4, 8), (4, 1, 1, 0), (4, 1, 1, 1025), (41, 1, 1, 8)):
        assert _verify_raw(field, bad, shift, seed, root, (list(z) + [0] * 40)[:max(bad[0], 1)], v, proof) == (BAD, -7), bad
    assert _verify_raw(field, case, 0, seed, root, z, v, proof) == (BAD, -7)
    assert _verify_raw(field, case, shift, seed, root, z, v, proof, raw_shift=_raw(p)) == (BAD, -7)
    assert _verify_raw(field, case, shift, seed, root, z, v, proof, raw_value=_raw(p)) == (BAD, -7)
    unreduced = np.ascontiguousarray(orc.from_ints(field, list(z)))
    unreduced[2] = _raw(p)
    assert _verify_raw(field, case, shift, seed, root, z, v, proof, raw_point=unreduced) == (BAD, -7)
    assert _verify_raw(field, case, shift, seed, root, z, v, proof, proof_len=len(proof) - 32) == (BAD, -7)
    two = orc.two_adicity(field) if hasattr(orc, "two_adicity") else zk_amd.two_adicity(field)
    big = (two, 1, 0, 1)   # n + b one past the two-adicity; the length is checked first, so the buffer has that length
    if two <= 40:
        buf = bytes(ref.proof_bytes(*big))
        assert _verify_raw(field, big, shift, seed, root, [0] * two, v, buf) == (NO_ROOT, -7)
    n = c.c_uint64(5)
    for bad in ((0, 1, 0, 8), (4, 0, 1, 8), (4, 9, 1, 8), (4, 1, 4, 8), (4, 1, 1, 0), (4, 1, 1, 1025)):
        assert _lib.lib.zk_mlpcs_proof_bytes(*bad, c.byref(n)) == BAD and n.value == 5, bad
    assert _lib.lib.zk_mlpcs_proof_bytes(4, 1, 1, 8, None) == BAD
    assert _lib.lib.zk_mlpcs_free(None) == 0
