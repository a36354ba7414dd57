"""The definition of the wiring permutation argument (tests/perm_ref.py) checked on its own, and the host side of the library against it
without a GPU: perm_ref accepts satisfied wiring and rejects one broken copy, a != b, each of the 2 k values altered, a non-canonical
element and a verifier that drops the padding columns' contribution; the head of its proof is gprod_ref.prove on its fingerprint table
under seed'; zk_perm_verify_host on the shared cases of the three fields (accepted proofs give the definition's point and claims, on a
rejection nothing is written); the error table; zk_perm_proof_bytes; the verifier at N = 40; wiring_sigma; the new exports and their
Python signatures.  Everything is bytes."""
import ctypes as c
import os
import random
import re
import resource
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gprod_ref  # noqa: E402
import perm_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, BAD_FIELD = -20, -21
SYMBOLS = ("zk_perm_proof_bytes", "zk_mle_perm_fingerprint", "zk_perm_prove", "zk_perm_verify_host", "zk_bench_perm")
WRAPPERS = ("perm_fingerprint", "permutation_prove", "permutation_verify", "perm_proof_bytes", "bench_perm", "wiring_sigma")
UNTOUCHED = 0x0909090909090909


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _raw(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def _verify_raw(field, n, k, beta, gamma, seed, proof, proof_len=None, raw_beta=None, raw_gamma=None):
    """(status, ok, point, claims): ints when accepted, else whether the buffers were left alone"""
    ok = c.c_int32(-7)
    point, claims = np.full((41, 4), UNTOUCHED, dtype=np.uint64), np.full((33, 4), UNTOUCHED, dtype=np.uint64)
    sd, pf = _u8(seed), _u8(proof)
    bv = raw_beta if raw_beta is not None else orc.from_int(field if field in (0, 1, 2) else 0, beta)
    gv = raw_gamma if raw_gamma is not None else orc.from_int(field if field in (0, 1, 2) else 0, gamma)
    rc = _lib.lib.zk_perm_verify_host(field, n, k, bv.ctypes.data_as(_lib.u64p), gv.ctypes.data_as(_lib.u64p), sd.ctypes.data_as(_lib.u8p),
                                      pf.ctypes.data_as(_lib.u8p), len(proof) if proof_len is None else proof_len,
                                      point.ctypes.data_as(_lib.u64p), claims.ctypes.data_as(_lib.u64p), c.byref(ok))
    if rc == 0 and ok.value == 1:
        assert (point[n:] == UNTOUCHED).all() and (claims[2 * k:] == UNTOUCHED).all()
        return rc, 1, orc.to_ints(field, point[:n]), orc.to_ints(field, claims[:2 * k])
    return rc, ok.value, bool((point == UNTOUCHED).all()), bool((claims == UNTOUCHED).all())


def _both(field, n, k, beta, gamma, seed, proof):
    rc, ok, point, claims = _verify_raw(field, n, k, beta, gamma, seed, proof)
    want = ref.verify(field, n, k, beta, gamma, seed, proof)
    assert rc == 0 and ok == int(want is not None), (n, k, rc, ok, want)
    if want is None:
        assert point is True and claims is True   # nothing was written
        return None
    assert (point, claims) == (list(want[0]), list(want[1]))
    return want


def _put(proof, at, value):
    return proof[:at] + int(value).to_bytes(32, "big") + proof[at + 32:]


@pytest.fixture(scope="module")
def proofs():
    """{case: (field, w, sigma, beta, gamma, seed, proof, point, claims)} from the definition, computed once"""
    out = {}
    for case in ref.HOST_CASES:
        inputs = ref.case_inputs(case, worst_case_values)
        out[case] = inputs + ref.prove(*inputs)
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
    assert re.search(r"^OBJS := .*\bperm\.o\b", make, flags=re.M)
    for switch in ("ZK_PERM_FUSE", "ZK_PERM_MAX_GRID"):
        assert switch in header, switch


def test_case_lists():
    assert {(cs[0], cs[1]) for cs in ref.HOST_CASES} >= {(1, 1), (2, 1), (3, 2), (2, 3), (3, 5), (4, 8), (6, 3)}
    assert {ref.case_field(cs) for cs in ref.HOST_CASES} == {0, 1, 2} and {cs[3] for cs in ref.HOST_CASES} == {0, 1}
    assert {ref.kappa(cs[1]) for cs in ref.HOST_CASES} == {0, 1, 2, 3, 4}
    assert [ref.kappa(k) for k in (1, 2, 3, 4, 5, 8, 9, 16)] == [0, 1, 2, 2, 3, 3, 4, 4]
    core = open(os.path.join(ROOT, "zk_amd", "csrc", "host_core.hpp")).read()
    assert ref.MAX_VARS == int(re.search(r"constexpr uint64_t kMaxVars = (\d+);", core).group(1))


def test_the_definition_on_its_own(proofs):
    for case, (field, w, sigma, beta, gamma, seed, proof, point, claims) in proofs.items():
        n, k, p = case[0], case[1], orc.modulus(field)
        N = ref.total_vars(n, k)
        assert len(proof) == ref.proof_bytes(n, k) == 32 * (2 * N * N + 2 * k), case
        assert [gprod_ref.evaluate(t, point, p) for t in w + sigma] == claims, case   # the claims that are left are true
        # the head is the grand product's proof of the materialised table under seed', its level 1 the two side products
        F = ref.fingerprint(field, w, sigma, beta, gamma)
        assert len(F) == 1 << N
        prod, head, r, claim = gprod_ref.prove(field, F, ref.seed_prime(field, n, k, beta, gamma, seed))
        assert head == proof[:gprod_ref.proof_bytes(N)] and r[ref.kappa(k):ref.kappa(k) + n] == point, case
        a, b = (int.from_bytes(proof[i:i + 32], "big") for i in (0, 32))
        ident, sig = 1, 1
        for v in range(len(F) // 2):
            ident, sig = ident * F[2 * v] % p, sig * F[2 * v + 1] % p
        assert (a, b) == (ident, sig) and prod == a * b % p and claim == gprod_ref.evaluate(F, r, p), case
        got = ref.verify(field, n, k, beta, gamma, seed, proof)
        if case[3]:
            assert a != b and got is None, case   # one broken copy
            continue
        assert a == b and got == (point, claims), case
        # a != b: the pair replaced by another one with the same product
        two = pow(2, p - 2, p)
        assert ref.verify(field, n, k, beta, gamma, seed, _put(_put(proof, 0, a * 2 % p), 32, b * two % p)) is None, case
        base = gprod_ref.proof_bytes(N)
        for i in range(2 * k):   # each of the 2 k values
            at = base + 32 * i
            assert ref.verify(field, n, k, beta, gamma, seed, _put(proof, at, (claims[i] + 1) % p)) is None, (case, i)
        for at in (0, base - 32, base, len(proof) - 32):   # a non-canonical element
            assert ref.verify(field, n, k, beta, gamma, seed, _put(proof, at, p)) is None, (case, at)
        # the padding columns' ones belong to the closing equation
        dropped = ref.verify(field, n, k, beta, gamma, seed, proof, drop_padding=True)
        assert (dropped is None) == (k != 1 << ref.kappa(k)), case
        assert ref.verify(field, n, k, (beta + 1) % p, gamma, seed, proof) is None and ref.verify(field, n, k, beta, (gamma + 1) % p, seed, proof) is None


def test_verify_host_against_the_definition(proofs):
    for case, (field, w, sigma, beta, gamma, seed, proof, point, claims) in proofs.items():
        n, k, p = case[0], case[1], orc.modulus(field)
        assert len(proof) == zk_amd.perm_proof_bytes(n, k), case
        got = _both(field, n, k, beta, gamma, seed, proof)
        bv, gv = orc.from_int(field, beta), orc.from_int(field, gamma)
        out = zk_amd.permutation_verify(field, n, k, bv, gv, seed, proof)
        if case[3]:
            assert got is None and out is None, case
            continue
        assert got == (point, claims), case
        assert out is not None and orc.to_ints(field, out[0]) == point and orc.to_ints(field, out[1]) == claims
        for name, at in ref.section_offsets(n, k).items():
            if at + 32 > len(proof) or (name in gprod_ref.section_offsets(3) and ref.total_vars(n, k) < 3):
                continue
            bad = bytearray(proof)
            bad[at + 31] ^= 1
            assert _both(field, n, k, beta, gamma, seed, bytes(bad)) is None, (case, name)
            assert _both(field, n, k, beta, gamma, seed, _put(proof, at, p)) is None, (case, name)            # an element >= p
            assert _both(field, n, k, beta, gamma, seed, _put(proof, at, (1 << 256) - 1)) is None, (case, name)
        a = int.from_bytes(proof[:32], "big")
        two = pow(2, p - 2, p)
        assert _both(field, n, k, beta, gamma, seed, _put(_put(proof, 0, a * 2 % p), 32, a * two % p)) is None, case   # a != b, the same product
        assert _both(field, n, k, beta, gamma, bytes([seed[0] ^ 1]) + seed[1:], proof) is None, case
        assert _both(field, n, k, (beta + 1) % p, gamma, seed, proof) is None and _both(field, n, k, beta, (gamma + 1) % p, seed, proof) is None
        for other in (proof[:-1], proof + b"\0", proof[:-32], proof + proof[-32:]):
            assert ref.verify(field, n, k, beta, gamma, seed, other) is None
            assert _verify_raw(field, n, k, beta, gamma, seed, other) == (BAD, -7, True, True)


def test_verifier_argument_table_and_proof_bytes(proofs):
    case = (3, 5, 0, 0)
    field, w, sigma, beta, gamma, seed, proof, point, claims = proofs[case]
    n, k, p = case[0], case[1], orc.modulus(field)
    assert _verify_raw(field, n, k, beta, gamma, seed, proof)[:2] == (0, 1)
    sd, pf = _u8(seed), _u8(proof)
    bv, gv = orc.from_int(field, beta), orc.from_int(field, gamma)
    pt, cl, ok = np.full((n, 4), UNTOUCHED, dtype=np.uint64), np.full((2 * k, 4), UNTOUCHED, dtype=np.uint64), c.c_int32(-7)
    args = [field, n, k, bv.ctypes.data_as(_lib.u64p), gv.ctypes.data_as(_lib.u64p), sd.ctypes.data_as(_lib.u8p), pf.ctypes.data_as(_lib.u8p), len(proof),
            pt.ctypes.data_as(_lib.u64p), cl.ctypes.data_as(_lib.u64p), c.byref(ok)]
    for i in (3, 4, 5, 6, 8, 9, 10):
        bad = list(args)
        bad[i] = None
        assert _lib.lib.zk_perm_verify_host(*bad) == BAD, i
    bad = list(args)
    bad[0], bad[3] = 7, None
    assert _lib.lib.zk_perm_verify_host(*bad) == BAD            # a NULL before the field
    assert (pt == UNTOUCHED).all() and (cl == UNTOUCHED).all() and ok.value == -7
    assert _verify_raw(7, 0, 0, beta, gamma, seed, proof) == (BAD_FIELD, -7, True, True)   # the field before the shapes
    for bad_n, bad_k in ((0, k), (n, 0), (n, 17), (40, 1), (36, 16), (n - 1, k), (n + 1, k), (n, k + 1)):
        assert _verify_raw(field, bad_n, bad_k, beta, gamma, seed, proof) == (BAD, -7, True, True), (bad_n, bad_k)
    assert _verify_raw(field, n, k, beta, gamma, seed, proof, proof_len=len(proof) - 32) == (BAD, -7, True, True)
    assert _verify_raw(field, n, k, beta, gamma, seed, proof, raw_beta=_raw(p)) == (BAD, -7, True, True)      # beta not reduced
    assert _verify_raw(field, n, k, beta, gamma, seed, proof, raw_gamma=_raw(p + 1)) == (BAD, -7, True, True)
    out = c.c_uint64(5)
    pb = _lib.lib.zk_perm_proof_bytes
    for bad_n, bad_k in ((0, 1), (4, 0), (4, 17), (40, 1), (39, 2), (36, 9), (1 << 31, 1), (4, 1 << 31)):
        assert pb(bad_n, bad_k, c.byref(out)) == BAD and out.value == 5, (bad_n, bad_k)
    assert pb(4, 3, None) == BAD
    for good_n, good_k, N in ((39, 1, 40), (38, 2, 40), (35, 16, 40), (36, 8, 40), (1, 1, 2)):
        assert pb(good_n, good_k, c.byref(out)) == 0 and out.value == 32 * (2 * N * N + 2 * good_k) == ref.proof_bytes(good_n, good_k)
    with pytest.raises(zk_amd.ZkError):
        zk_amd.perm_proof_bytes(0, 1)


def test_verifier_at_forty_variables_allocates_nothing_sized_by_n():
    """N = 40 (n = 35, k = 16; a column of 2^35 elements would be 1 TiB): the verifier runs and gives the definition's verdict.  A proof of
    zeros has a = b = 0 and passes every sumcheck round with the claim 0, so the verdict hangs on the closing equation: with beta,
    gamma != 0 it does not hold, with beta = gamma = 0 and no padding column (k = 16) it does; the process's peak memory does not move"""
    field, n, k = zk_amd.BLS12_381_FR, 35, 16
    p = orc.modulus(field)
    proof = bytes(ref.proof_bytes(n, k))
    seed = bytes(range(32))
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    assert _both(field, n, k, 5, 7, seed, proof) is None
    want = _both(field, n, k, 0, 0, seed, proof)
    assert want is not None and want[1] == [0] * 32 and len(want[0]) == n
    assert _both(field, n, k, 0, 0, seed, _put(proof, len(proof) - 32, 1)) is not None   # a sigma value: beta = 0 hides it
    assert _both(field, n, k, 0, 0, seed, _put(proof, len(proof) - 32 * 17, 1)) is None  # a w value does not hide
    assert _both(field, n, k, 0, 0, seed, _put(proof, 32 * 5, 1)) is None
    assert _both(field, 38, 1, 0, 0, seed, bytes(ref.proof_bytes(38, 1))) is not None
    assert resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before < 64 * 1024   # KiB


def test_wiring_sigma_is_a_permutation_that_cycles_every_class():
    rng = random.Random(5)
    for k, n, n_classes in ((1, 1, 1), (1, 3, 3), (3, 4, 10), (5, 5, 200), (16, 3, 7), (2, 6, 1)):
        classes = np.array([[rng.randrange(n_classes) * 7 - 3 for _ in range(1 << n)] for _ in range(k)])
        sigma = zk_amd.wiring_sigma(classes)
        assert sigma.shape == classes.shape and sigma.dtype == np.uint64
        flat_c, flat_s = classes.reshape(-1), sigma.reshape(-1).astype(np.int64)
        assert sorted(flat_s.tolist()) == list(range(k << n))                 # a permutation of the labels
        assert (flat_c[flat_s] == flat_c).all()                               # inside the classes
        assert sigma.tolist() == ref.wiring_sigma(classes.tolist())           # the definition's cycles: ascending labels, the last to the first
        for cid in set(flat_c.tolist()):                                      # one cycle per class
            members = np.flatnonzero(flat_c == cid)
            at, seen = members[0], 0
            for _ in range(len(members)):
                at, seen = flat_s[at], seen + 1
            assert at == members[0] and len({int(x) for x in members}) == seen
    with pytest.raises(zk_amd.ZkError):
        zk_amd.wiring_sigma(np.zeros((0, 4)))
    with pytest.raises(zk_amd.ZkError):
        zk_amd.wiring_sigma([1, 2, 3])
