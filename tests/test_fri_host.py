"""The definition of the FRI low-degree proofs (tests/fri_ref.py) checked on its own, the host verifier zk_fri_verify_host against it on the
shared case list (accepted proofs, one flipped bit in every section, changed seed / shift / parameters, layers that are not low-degree),
the error table, zk_fri_proof_bytes, the new exports and their Python signatures -- all without a GPU.  Everything is bit-exact."""
import ctypes as c
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import ZkError, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
EVAL_LEN, NO_ROOT, BAD, BAD_FIELD = -1, -7, -20, -21
SYMBOLS = ("zk_fri_lde", "zk_fri_fold", "zk_fri_proof_bytes", "zk_fri_prove", "zk_fri_verify_host", "zk_bench_fri_fold")
WRAPPERS = ("fri_lde", "fri_fold", "fri_prove", "fri_verify", "fri_proof_bytes")


def _no_gpu():
    n = c.c_int32()
    _lib.lib.zk_device_count(c.byref(n))
    return n.value == 0


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _verify_raw(field, case, shift, seed, proof, proof_len=None):
    """(status, ok) of zk_fri_verify_host on raw buffers; shift: a canonical int"""
    d, b, a, f, q = case
    ok = c.c_int32(-7)
    sv, sd, pv = orc.from_int(field, shift), _u8(seed), _u8(proof)
    rc = _lib.lib.zk_fri_verify_host(field, d, b, a, f, q, sv.ctypes.data_as(_lib.u64p), sd.ctypes.data_as(_lib.u8p), pv.ctypes.data_as(_lib.u8p),
                                     len(proof) if proof_len is None else proof_len, c.byref(ok))
    return rc, ok.value


def _flip(b, byte, bit):
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


@pytest.fixture(scope="module")
def proofs():
    """{case: (field, coefficients, shift, seed, the definition's proof)} for the shared case list, computed once"""
    out = {}
    for case in ref.CASES:
        field = ref.case_field(case)
        coeffs, shift, seed = ref.case_inputs(field, case)
        out[case] = (field, coeffs, shift, seed, ref.prove(field, coeffs, *case, shift, seed))
    return out


def test_exports_signatures_and_abi_version():
    assert _lib.lib.zk_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    assert "#define ZK_AMD_ABI_VERSION 6" in header
    for name in SYMBOLS:
        assert hasattr(_lib.lib, name), name
        assert name in _lib._sig and name in _lib.declared_symbols(), name
        assert re.search(r"\bint32_t %s\(" % name, header), name
    for name in WRAPPERS:
        assert name in zk_amd.api.__all__ and hasattr(zk_amd, name), name


def test_case_lists():
    assert all(2 <= d <= 10 and 1 <= b <= 3 and 1 <= a <= 3 and 0 <= f <= 2 and f < d and (d - f) % a == 0 and q in (1, 8) for d, b, a, f, q in ref.CASES)
    want = sum(1 for d in range(2, 11) for b in (1, 2, 3) for a in (1, 2, 3) for f in (0, 1, 2) if f < d and (d - f) % a == 0) * 2
    assert len(ref.CASES) == len(set(ref.CASES)) == want
    assert {c[2] for c in ref.CASES} == {1, 2, 3} and {ref.case_field(c) for c in ref.CASES} == {0, 1, 2}
    assert set(ref.GPU_CASES) - set(ref.CASES) == set(ref.GPU_EXTRA_CASES) and max(c[0] for c in ref.GPU_CASES) == 12
    assert ref.fold_logs(2) == (2, 3, 6, 7, 8, 9, 12, 13, 14)


@pytest.mark.parametrize("fi", range(3), ids=ref.FIELD_IDS)
def test_fold_of_an_lde_is_the_lde_of_the_folded_coefficients(fi):
    """fold(lde(c)) = lde of c'[m] = sum_j beta^j c[2^a m + j] on the shift^(2^a) coset: a = 1..3, d <= 6, shifts 1, 5, p - 1, beta in
    {0, 1, p - 1, random}; and fold2 against its formula on one pair"""
    p = orc.modulus(fi)
    rng = random.Random(0xF0 + fi)
    for a in (1, 2, 3):
        for d in range(a, 7):
            coeffs = [rng.randrange(p) for _ in range(1 << d)]
            for name in ref.SHIFTS:
                s = ref.shift_value(p, name)
                ev = ref.lde(fi, coeffs, d + 1, s)
                for beta in ref.betas(p, rng):
                    folded = [sum(pow(beta, j, p) * coeffs[(m << a) + j] for j in range(1 << a)) % p for m in range(1 << (d - a))]
                    assert ref.fold(fi, ev, s, beta, a) == ref.lde(fi, folded, d + 1 - a, pow(s, 1 << a, p)), (a, d, name, beta)
    v, s, beta = [3, 7], 5, 11
    w = ref.root(fi, 2)
    assert w == p - 1
    assert ref.fold2(fi, v, s, beta) == [((3 + 7) * pow(2, p - 2, p) + beta * (3 - 7) * pow(2 * s, p - 2, p)) % p]
    # the transform is the plain sum and its inverse undoes it
    co = [rng.randrange(p) for _ in range(8)]
    w8 = ref.root(fi, 8)
    assert ref.fft(fi, co) == [sum(cj * pow(w8, j * k, p) for j, cj in enumerate(co)) % p for k in range(8)]
    assert ref.fft(fi, ref.fft(fi, co), inverse=True) == co
    assert orc.to_ints(fi, orc.fft(fi, orc.from_ints(fi, co))) == ref.fft(fi, co)


@pytest.mark.parametrize("fi", range(3), ids=ref.FIELD_IDS)
def test_fold_at_is_one_output_of_fold(fi):
    """fold_at (the sampled reference of the folds too large to fold whole in Python) against fold(...)[i] for every i: a = 1..3,
    2^a, 2^(a+1) and 2^6 points, shifts 1, 5, p - 1 and a random one, beta in {0, 1, p - 1, random}; it reads the 2^a inputs
    i + j M and no other"""
    p = orc.modulus(fi)
    rng = random.Random(0xA7 + fi)
    for a in (1, 2, 3):
        for log_n in (a, a + 1, 6):
            v = [rng.randrange(p) for _ in range(1 << log_n)]
            v[0], v[-1] = 0, p - 1
            m = 1 << (log_n - a)
            for s in (1, 5, p - 1, rng.randrange(1, p)):
                for beta in ref.betas(p, rng):
                    want = ref.fold(fi, v, s, beta, a)
                    assert len(want) == m
                    for i in range(m):
                        read = []
                        got = ref.fold_at(fi, lambda idx: (read.append(idx), v[idx])[1], log_n, s, beta, a, i)
                        assert got == want[i], (a, log_n, s, beta, i)
                        assert sorted(read) == [i + j * m for j in range(1 << a)], (a, log_n, i)


@pytest.mark.parametrize("fi", range(3), ids=ref.FIELD_IDS)
def test_fold_of_the_even_and_of_the_odd_inputs(fi):
    """what the GPU test of the folds with more than 2^23 outputs relies on: the even outputs of a fold are the fold of the even inputs
    (the coset of s over w^2), the odd outputs the fold of the odd inputs (the coset of s w); a = 1..3, 16 to 128 points"""
    p = orc.modulus(fi)
    rng = random.Random(0xE0DD + fi)
    for a in (1, 2, 3):
        for log_n in range(4, 8):
            v = [rng.randrange(p) for _ in range(1 << log_n)]
            w = ref.root(fi, 1 << log_n)
            for s in (1, 5, p - 1, rng.randrange(1, p)):
                beta = ref.betas(p, rng)[(a + log_n) % 4]
                whole = ref.fold(fi, v, s, beta, a)
                assert whole[0::2] == ref.fold(fi, v[0::2], s, beta, a), (a, log_n, s, "even")
                assert whole[1::2] == ref.fold(fi, v[1::2], s * w % p, beta, a), (a, log_n, s, "odd")
                assert whole[1::2] != ref.fold(fi, v[1::2], s, beta, a) or beta == 0, (a, log_n, s, "the shift of the odd half matters")


def test_large_case_lists():
    """the large folds have 2^24 outputs (the first size at which k_fri_fold's loop takes a second trip: fri.hip caps its grid at
    2 * kMaxGridStream workgroups of 256 outputs), FOLD_LOG_LARGE does not, and the large proofs have a layer 0 of 2^22 points"""
    host = open(os.path.join(ROOT, "zk_amd", "csrc", "fri.hip")).read()
    core = open(os.path.join(ROOT, "zk_amd", "csrc", "host_core.hpp")).read()
    assert "if (g > 2 * kMaxGridStream) g = 2 * kMaxGridStream;" in host
    per_sweep = 2 * int(re.search(r"constexpr uint32_t kMaxGridStream = (\d+);", core).group(1)) * 256
    assert per_sweep == 1 << 23
    assert all(1 << (log_n - a) == 2 * per_sweep for a, log_n, _ in ref.FOLD_BIG)
    assert all(1 << (ref.FOLD_LOG_LARGE - a) < per_sweep for a in (1, 2, 3))
    assert {a for a, _, _ in ref.FOLD_BIG} == {1, 3} and all(log_n <= orc.two_adicity(0) for _, log_n, _ in ref.FOLD_BIG)
    assert all(d + b == 22 and f == 0 and q == 8 and (d - f) % a == 0 for d, b, a, f, q in ref.PROOF_BIG)
    idx = ref.fold_big_samples(1 << 24)
    assert len(idx) == len(set(idx)) == ref.FOLD_BIG_SAMPLES and max(idx) == (1 << 24) - 1 and min(idx) == 0
    assert {63, 64}.union(range((1 << 23) - 64, (1 << 23) + 65)) <= set(idx)


def test_definition_accepts_its_own_proofs(proofs):
    for case in ref.CASES[::7]:
        field, _, shift, seed, proof = proofs[case]
        assert len(proof) == ref.proof_bytes(*case)
        assert ref.verify(field, proof, *case, shift, seed), case
        assert not ref.verify(field, _flip(proof, 5, 0), *case, shift, seed), case


def test_proof_bytes_against_the_formula():
    n = c.c_uint64()
    for d, b, a, f, q in ref.CASES + ((40, 8, 1, 0, 1024), (12, 8, 3, 0, 1024)):
        rounds = (d - f) // a
        want = 32 * (rounds + 2 ** f + q * sum(2 ** a + (d + b - a * r - a) for r in range(rounds)))
        assert _lib.lib.zk_fri_proof_bytes(d, b, a, f, q, c.byref(n)) == 0 and n.value == want == ref.proof_bytes(d, b, a, f, q)
        assert zk_amd.fri_proof_bytes(d, b, a, f, q) == want
    n.value = 77
    for bad in ((8, 2, 0, 0, 8), (8, 2, 4, 0, 8), (8, 0, 2, 0, 8), (8, 9, 2, 0, 8), (8, 2, 2, 0, 0), (8, 2, 2, 0, 1025), (8, 2, 2, 8, 8), (2, 2, 1, 3, 8),
                (8, 2, 3, 0, 8), (41, 2, 1, 0, 8)):
        assert _lib.lib.zk_fri_proof_bytes(*bad, c.byref(n)) == BAD, bad
    assert _lib.lib.zk_fri_proof_bytes(8, 2, 2, 0, 8, None) == BAD and n.value == 77


def test_verify_host_accepts_the_definitions_proofs(proofs):
    """every (d, b, a, f, Q) of the shared list, the field and the shift rotating over the cases"""
    for case in ref.CASES:
        field, _, shift, seed, proof = proofs[case]
        assert _verify_raw(field, case, shift, seed, proof) == (0, 1), case
    case = ref.CASES[-1]
    field, _, shift, seed, proof = proofs[case]
    assert zk_amd.fri_verify(field, proof, *case, orc.from_int(field, shift), seed)


def _sections(case):
    """[(name, first byte, length)] of every section of a proof: each root, each final coefficient, each row element and each path node of
    every query and round"""
    d, b, a, f, q = case
    rounds = (d - f) // a
    out = [("root", 32 * r, 32) for r in range(rounds)] + [("final", 32 * (rounds + j), 32) for j in range(1 << f)]
    at = 32 * (rounds + (1 << f))
    for _ in range(q):
        for r in range(rounds):
            out += [("row", at + 32 * j, 32) for j in range(1 << a)]
            at += 32 << a
            m = d + b - a * r - a
            out += [("path", at + 32 * j, 32) for j in range(m)]
            at += 32 * m
    assert at == ref.proof_bytes(*case)
    return out


def test_verify_host_rejects_every_flipped_section_and_changed_statement(proofs):
    """one bit flipped in every root, final coefficient, row element and path node, for every query and round, on the cases with d <= 7
    and on three larger ones; a changed seed, shift, field or parameter; the definition gives the same verdict on a sample"""
    rng = random.Random(0xF11B)
    cases = [cs for cs in ref.CASES if cs[0] <= 7] + [(10, 3, 1, 0, 8), (10, 2, 2, 2, 8), (9, 1, 3, 0, 8)]
    for case in cases:
        field, _, shift, seed, proof = proofs[case]
        p = orc.modulus(field)
        for k, (name, first, length) in enumerate(_sections(case)):
            bad = _flip(proof, first + rng.randrange(length), rng.randrange(8))
            assert _verify_raw(field, case, shift, seed, bad) == (0, 0), (case, name, first)
            if k % 97 == 0:
                assert not ref.verify(field, bad, *case, shift, seed), (case, name, first)
        assert _verify_raw(field, case, shift, _flip(seed, 31, 0), proof) == (0, 0), case
        assert _verify_raw(field, case, shift % (p - 1) + 1, seed, proof) == (0, 0), case
        assert _verify_raw((field + 1) % 3, case, shift % orc.modulus((field + 1) % 3) or 1, seed, proof) == (0, 0), case
        d, b, a, f, q = case
        for other in ((d, b + 1, a, f, q), (d, b, a, f, q + 1), (d + a, b, a, f, q), (d + 1, b - 1, a, f + 1, q)):
            rc, ok = _verify_raw(field, other, shift, seed, proof)
            assert rc == BAD or (rc, ok) == (0, 0), (case, other)   # another length, or the same length and another transcript
    # elements that are not canonical are a verdict, not an error: the modulus itself as a final coefficient and as a row element
    case = (4, 1, 2, 0, 1)
    field, _, shift, seed, proof = proofs[case]
    p = orc.modulus(field)
    for name, first, _ in _sections(case):
        if name in ("final", "row"):
            bad = proof[:first] + ((1 << 256) - 1 if name == "row" else p).to_bytes(32, "big") + proof[first + 32:]
            assert _verify_raw(field, case, shift, seed, bad) == (0, 0) and not ref.verify(field, bad, *case, shift, seed), (name, first)


@pytest.mark.parametrize("fi", range(3), ids=ref.FIELD_IDS)
def test_verify_host_agrees_with_the_definition_on_layers_that_are_not_low_degree(fi):
    """prove_evals on a random vector, on the LDE of a polynomial of 2^d + 1 coefficients and on a valid LDE with one value changed at a
    queried index: seeds are tried in order until the definition rejects, and the library gives the definition's verdict on every one"""
    p = orc.modulus(fi)
    rng = random.Random(0xBAD + fi)
    rejected = 0
    for case in ((3, 1, 1, 0, 8), (4, 2, 2, 0, 8), (6, 1, 3, 0, 8), (5, 2, 1, 1, 8), (6, 3, 2, 2, 8)):
        d, b, a, f, q = case
        n0 = 1 << (d + b)
        shift = (5, p - 1, 1)[fi]
        good = ref.lde(fi, [rng.randrange(p) for _ in range(1 << d)], d + b, shift)
        over = ref.lde(fi, [rng.randrange(1, p) for _ in range((1 << d) + 1)], d + b, shift)
        layers = {"random": lambda seed: [rng.randrange(p) for _ in range(n0)], "one_more_coefficient": lambda seed: over}

        def planted(seed):
            honest = ref.prove_evals(fi, good, *case, shift, seed)
            idx = ref.query_indices(fi, honest, *case, shift, seed)[0]
            changed = list(good)
            at = idx + (rng.randrange(1 << a) << (d + b - a))
            changed[at] = (changed[at] + 1 + rng.randrange(p - 1)) % p
            return changed

        layers["changed_at_a_queried_index"] = planted
        for name, make in layers.items():
            for k in range(64):
                seed = bytes([fi, k, d, b, a, f]) + bytes(26)
                proof = ref.prove_evals(fi, make(seed), *case, shift, seed)
                want = ref.verify(fi, proof, *case, shift, seed)
                assert _verify_raw(fi, case, shift, seed, proof) == (0, int(want)), (case, name, k)
                if not want:
                    rejected += 1
                    break
            else:
                raise AssertionError(f"no seed of 64 makes the definition reject {name} {case}")
        seed = bytes(32)
        assert ref.verify(fi, ref.prove_evals(fi, good, *case, shift, seed), *case, shift, seed)
    assert rejected == 15


def test_verify_host_error_table(proofs):
    lib = _lib.lib
    case = (4, 1, 2, 0, 1)
    field, _, shift, seed, proof = proofs[case]
    p = orc.modulus(field)
    d, b, a, f, q = case
    ok = c.c_int32(-7)
    sv, sd, pv = orc.from_int(field, shift), _u8(seed), _u8(proof)
    sp, dp, pp, n = sv.ctypes.data_as(_lib.u64p), sd.ctypes.data_as(_lib.u8p), pv.ctypes.data_as(_lib.u8p), len(proof)
    assert lib.zk_fri_verify_host(field, d, b, a, f, q, sp, dp, pp, n, c.byref(ok)) == 0 and ok.value == 1
    ok.value = -7
    assert lib.zk_fri_verify_host(field, d, b, a, f, q, None, dp, pp, n, c.byref(ok)) == BAD
    assert lib.zk_fri_verify_host(field, d, b, a, f, q, sp, None, pp, n, c.byref(ok)) == BAD
    assert lib.zk_fri_verify_host(field, d, b, a, f, q, sp, dp, None, n, c.byref(ok)) == BAD
    assert lib.zk_fri_verify_host(field, d, b, a, f, q, sp, dp, pp, n, None) == BAD
    assert lib.zk_fri_verify_host(9, d, b, a, f, q, None, dp, pp, n, c.byref(ok)) == BAD          # the NULL is seen first
    assert lib.zk_fri_verify_host(9, d, b, a, f, q, sp, dp, pp, n, c.byref(ok)) == BAD_FIELD
    assert lib.zk_fri_verify_host(9, d, b, 0, f, q, sp, dp, pp, n, c.byref(ok)) == BAD_FIELD      # the field before the parameters
    for bad in ((d, b, 0, f, q), (d, b, 4, f, q), (d, 0, a, f, q), (d, 9, a, f, q), (d, b, a, f, 0), (d, b, a, f, 1025), (d, b, a, d, q),
                (d, b, a, d + 1, q), (d, b, 3, f, q), (41, b, 1, f, q)):
        assert lib.zk_fri_verify_host(field, *bad, sp, dp, pp, n, c.byref(ok)) == BAD, bad
    # the shift: zero, the modulus itself and all ones are refused (as zk_fe_from_canonical refuses the latter two)
    for v in (0, p, (1 << 256) - 1):
        raw = np.frombuffer(v.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
        assert lib.zk_fri_verify_host(field, d, b, a, f, q, raw.ctypes.data_as(_lib.u64p), dp, pp, n, c.byref(ok)) == BAD, v
    assert lib.zk_fri_verify_host(field, d, b, a, f, q, sp, dp, pp, n - 1, c.byref(ok)) == BAD
    assert lib.zk_fri_verify_host(field, d, b, a, f, q, sp, dp, pp, n + 32, c.byref(ok)) == BAD
    # a domain past the field's two-adicity (BN254: 2^28): the length is looked at first, so it has to fit
    big = (27, 2, 3, 0, 1)
    assert lib.zk_fri_verify_host(zk_amd.BN254_FR, *big, sp, dp, pp, ref.proof_bytes(*big), c.byref(ok)) in (NO_ROOT,)
    assert lib.zk_fri_verify_host(zk_amd.BN254_FR, *big, sp, dp, pp, n, c.byref(ok)) == BAD
    assert ok.value == -7   # nothing was written by any of them
    with pytest.raises(ZkError):
        zk_amd.fri_verify(field, proof, d, b, a, f, q, sv, seed[:-1])


def test_device_calls_reject_null_arguments_without_gpu():
    lib = _lib.lib
    fake = c.c_void_p(8)   # never dereferenced: a NULL among the others ends the call first
    h, ms = c.c_void_p(), c.c_double(-1.0)
    one = np.ones(4, dtype=np.uint64)
    ep = one.ctypes.data_as(_lib.u64p)
    buf = np.zeros(64, dtype=np.uint8)
    bp = buf.ctypes.data_as(_lib.u8p)
    assert lib.zk_fri_lde(None, fake, 3, ep, c.byref(h)) == BAD and lib.zk_fri_lde(fake, None, 3, ep, c.byref(h)) == BAD
    assert lib.zk_fri_lde(fake, fake, 3, None, c.byref(h)) == BAD and lib.zk_fri_lde(fake, fake, 3, ep, None) == BAD
    assert lib.zk_fri_fold(None, fake, 1, ep, ep, fake) == BAD and lib.zk_fri_fold(fake, None, 1, ep, ep, fake) == BAD
    assert lib.zk_fri_fold(fake, fake, 1, None, ep, fake) == BAD and lib.zk_fri_fold(fake, fake, 1, ep, None, fake) == BAD
    assert lib.zk_fri_fold(fake, fake, 1, ep, ep, None) == BAD
    assert lib.zk_fri_prove(None, fake, 4, 1, 2, 0, 1, ep, bp, bp) == BAD and lib.zk_fri_prove(fake, None, 4, 1, 2, 0, 1, ep, bp, bp) == BAD
    assert lib.zk_fri_prove(fake, fake, 4, 1, 2, 0, 1, None, bp, bp) == BAD and lib.zk_fri_prove(fake, fake, 4, 1, 2, 0, 1, ep, None, bp) == BAD
    assert lib.zk_fri_prove(fake, fake, 4, 1, 2, 0, 1, ep, bp, None) == BAD
    assert lib.zk_bench_fri_fold(None, fake, 1, fake, 0, 1, c.byref(ms)) == BAD and lib.zk_bench_fri_fold(fake, None, 1, fake, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_fri_fold(fake, fake, 1, None, 0, 1, c.byref(ms)) == BAD and lib.zk_bench_fri_fold(fake, fake, 1, fake, 0, 1, None) == BAD
    assert lib.zk_bench_fri_fold(fake, fake, 1, fake, 3, 1, c.byref(ms)) == BAD and lib.zk_bench_fri_fold(fake, fake, 1, fake, -1, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_fri_fold(fake, fake, 1, fake, 0, 0, c.byref(ms)) == BAD
    assert h.value is None and ms.value == -1.0 and not buf.any()


def test_switch_and_table_constants_match_the_source():
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "fri_kernels.cuh")).read()
    host = open(os.path.join(ROOT, "zk_amd", "csrc", "fri.hip")).read()
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    make = open(os.path.join(ROOT, "zk_amd", "csrc", "Makefile")).read()
    default = int(re.search(r"constexpr uint32_t kFriFusedDefault = (\d+);", host).group(1))
    assert re.search(r'env_u64\("ZK_FRI_FUSED_FOLD", kFriFusedDefault, 0, 1\)', host)
    assert re.search(r"ZK_FRI_FUSED_FOLD\s+%d\s+0 \.\. 1\b" % default, header)   # the switch's default and range
    assert int(re.search(r"constexpr uint32_t kFriMaxArityLog = (\d+);", src).group(1)) == 3
    # the sizes the GPU test folds straddle the split of the two-level power table
    split = int(re.search(r"constexpr uint32_t kFriTableLoBits = (\d+);", src).group(1))
    assert split in ref.FOLD_LOGS and split + 1 in ref.FOLD_LOGS
    assert re.search(r"^OBJS := .*\bfri\.o\b", make, flags=re.M)
    assert "asm" not in src   # plain C++ over field.cuh


def test_prove_without_gpu_fails_loudly():
    if not _no_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ZkError) as e:
        ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
        zk_amd.fri_prove(zk_amd.UnivariatePolynomial.new(ctx, np.zeros((2, 4), dtype=np.uint64)), 1, 1, 1, 0, 1, orc.from_int(0, 5), bytes(32))
    assert e.value.code == -22   # ZK_ERR_NO_DEVICE


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_fri")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fri.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    if not _no_gpu():
        pytest.skip("GPU present: run by tests/test_gpu_fri.py")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr
