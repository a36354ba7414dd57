"""The definition of the FRI polynomial commitment (tests/pcs_ref.py) checked on its own, and the host verifier zk_pcs_verify_host against
it on the shared case list: every honest proof accepted by both, every kind of change rejected by both, a polynomial over the degree
bound, zk_pcs_proof_bytes, the argument table, the new exports and their Python signatures -- all without a GPU.  Everything is bytes."""
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
import fri_ref  # noqa: E402
import pcs_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ROOT, BAD, BAD_FIELD = -7, -20, -21
SYMBOLS = ("zk_deep_quotient", "zk_pcs_commit", "zk_pcs_free", "zk_pcs_root", "zk_pcs_n_polys", "zk_pcs_proof_bytes", "zk_pcs_open",
           "zk_pcs_verify_host", "zk_bench_deep_quotient")
WRAPPERS = ("PolyCommitment", "pcs_verify", "pcs_proof_bytes", "deep_quotient")


def _no_gpu():
    n = c.c_int32()
    _lib.lib.zk_device_count(c.byref(n))
    return n.value == 0


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _raw(v):
    """limbs of an integer as they are, reduced or not"""
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def _verify_raw(field, case, shift, seed, root, z, ys, proof, proof_len=None):
    """(status, ok) of zk_pcs_verify_host on raw buffers; shift, z, ys: canonical ints"""
    k, d, b, a, f, q = case
    ok = c.c_int32(-7)
    sv, zv, yv = orc.from_int(field, shift), orc.from_int(field, z), np.ascontiguousarray(orc.from_ints(field, list(ys)))
    sd, rt, pv = _u8(seed), _u8(root), _u8(proof)
    rc = _lib.lib.zk_pcs_verify_host(field, len(ys), d, b, a, f, q, sv.ctypes.data_as(_lib.u64p), sd.ctypes.data_as(_lib.u8p), rt.ctypes.data_as(_lib.u8p),
                                     zv.ctypes.data_as(_lib.u64p), yv.ctypes.data_as(_lib.u64p), pv.ctypes.data_as(_lib.u8p),
                                     len(proof) if proof_len is None else proof_len, c.byref(ok))
    return rc, ok.value


def _both(field, case, shift, seed, root, z, ys, proof):
    """the verdict of the library and of the definition, which must be the same"""
    k, d, b, a, f, q = case
    rc, ok = _verify_raw(field, case, shift, seed, root, z, ys, proof)
    want = ref.verify(field, k, d, b, a, f, q, shift, seed, root, z, ys, proof)
    assert rc == 0 and ok == int(want), (case, rc, ok, want)
    return want


def _put(proof, at, value):
    return proof[:at] + int(value).to_bytes(32, "big") + proof[at + 32:]


@pytest.fixture(scope="module")
def proofs():
    """{case: (field, polys, shift, seed, z, root, ys, the definition's proof)} for the shared case list, computed once"""
    out = {}
    for case in ref.CASES:
        k, d, b, a, f, q = case
        field = ref.case_field(case)
        polys, shift, seed, z = ref.case_inputs(field, case)
        committed = ref.commit(field, polys, d, b, a, shift)
        ys, proof = ref.prove(field, polys, d, b, a, f, q, shift, seed, z, committed=committed)
        out[case] = (field, polys, shift, seed, z, ref.merkle_ref.root(committed[2]), ys, proof)
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
    assert re.search(r"^OBJS := .*\bpcs\.o\b", make, flags=re.M)


def test_case_lists_and_kernel_constants():
    want = {(k, d, b, a, f, q) for k in (1, 2, 5) for d in range(3, 9) for b in (1, 2) for a in (1, 2, 3) for f in (0, 1) for q in (1, 8) if (d - f) % a == 0}
    assert set(ref.CASES) == want and len(ref.CASES) == len(want)
    assert {ref.case_field(cs) for cs in ref.CASES} == {0, 1, 2}
    assert set(ref.GPU_CASES) == {cs for cs in ref.CASES if cs[5] == 8} | {(2, 11, 1, 3, 2, 8), (3, 12, 2, 2, 0, 8), (1, 12, 1, 1, 1, 1)}
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "pcs_kernels.cuh")).read()
    common = open(os.path.join(ROOT, "zk_amd", "csrc", "common.cuh")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    per = int(re.search(r"constexpr uint32_t kPcsPerThread = (\d+);", src).group(1))
    split = int(re.search(r"constexpr uint32_t kPcsTableLoBits = (\d+);", src).group(1))
    chunk_log = (block * per).bit_length() - 1
    assert block * per == 1 << chunk_log
    # exactly one chunk, two chunks = the split of the power table, and past both
    assert chunk_log in ref.QUOTIENT_LOGS and split in ref.QUOTIENT_LOGS and split + 1 in ref.QUOTIENT_LOGS and split == chunk_log + 1
    assert ref.QUOTIENT_LOGS == (1, 3, 6, 7, 11, 12, 13, 14) and ref.QUOTIENT_COLUMNS == (1, 2, 3, 5, 17)
    for log_n in ref.QUOTIENT_LOGS:   # the thinned product still names every value of every axis
        for k in ref.QUOTIENT_COLUMNS:
            combos = ref.quotient_combos(log_n, k)
            assert {s for s, _, _ in combos} == set(ref.SHIFTS) and {zi for _, zi, _ in combos} == {ai for _, _, ai in combos} == {0, 1, 2, 3}
    assert "asm" not in src   # plain C++ over field.cuh


@pytest.mark.parametrize("fi", range(3), ids=fri_ref.FIELD_IDS)
def test_quotient_of_right_values_is_low_degree_and_quotient_at_is_one_entry(fi):
    """q = sum_c alpha^c (f_c - y_c) / (X - z) as a polynomial: its evaluations over the coset interpolate to fewer than 2^d coefficients
    when y_c = f_c(z) and to a full vector when one y_c is off; quotient_at agrees with quotient at every index"""
    p = orc.modulus(fi)
    rng = random.Random(0x9C0 + fi)
    for k, d, b in ((1, 3, 1), (2, 4, 2), (5, 5, 1)):
        polys = [[rng.randrange(p) for _ in range(1 << d)] for _ in range(k)]
        for s in (1, 5, p - 1):
            z, alpha = rng.randrange(p), rng.randrange(p)
            while ref.on_domain(fi, d + b, s, z):
                z = rng.randrange(p)
            cols = [fri_ref.lde(fi, co, d + b, s) for co in polys]
            ys = [ref.evaluate(fi, co, z) for co in polys]
            quo = ref.quotient(fi, cols, s, z, ys, alpha)
            co = fri_ref.fft(fi, quo, inverse=True)
            sinv = pow(s, p - 2, p)
            assert all(x == 0 for x in co[(1 << d) - 1:]), (k, d, b, s)
            # the coefficients themselves: sum_c alpha^c (f_c - y_c) = q (X - z), with the shift taken out of the interpolant
            qc = [x * pow(sinv, j, p) % p for j, x in enumerate(co)][:1 << d]
            comb = [sum(pow(alpha, cc, p) * (polys[cc][j] - (ys[cc] if j == 0 else 0)) for cc in range(k)) % p for j in range(1 << d)]
            assert [((qc[j - 1] if j else 0) - z * qc[j]) % p for j in range(1 << d)] == comb
            for i in range(1 << (d + b)):
                assert ref.quotient_at(fi, lambda cc, i: cols[cc][i], k, d + b, s, z, ys, alpha, i) == quo[i]
            ys[-1] = (ys[-1] + 1) % p
            bad = fri_ref.fft(fi, ref.quotient(fi, cols, s, z, ys, alpha), inverse=True)
            assert any(bad[(1 << d):]), (k, d, b, s)
    assert ref.on_domain(fi, 4, 5, 5 * fri_ref.root(fi, 16) ** 5 % p) and not ref.on_domain(fi, 4, 5, 0) and ref.on_domain(fi, 3, 1, p - 1)


def test_proof_bytes_against_the_definition():
    n = c.c_uint64()
    for k, d, b, a, f, q in ref.CASES + ref.GPU_EXTRA_CASES + ((128, 40, 8, 3, 1, 1024), (512, 12, 8, 1, 0, 1)):
        want = fri_ref.proof_bytes(d, b, a, f, q) + 32 * q * ((k << a) + d + b - a)
        assert _lib.lib.zk_pcs_proof_bytes(k, d, b, a, f, q, c.byref(n)) == 0 and n.value == want == ref.proof_bytes(k, d, b, a, f, q)
        assert zk_amd.pcs_proof_bytes(k, d, b, a, f, q) == want
    n.value = 77
    for bad in ((0, 8, 2, 2, 0, 8), (2, 8, 2, 0, 0, 8), (2, 8, 2, 4, 0, 8), (2, 8, 0, 2, 0, 8), (2, 8, 9, 2, 0, 8), (2, 8, 2, 2, 0, 0), (2, 8, 2, 2, 0, 1025),
                (2, 8, 2, 2, 8, 8), (2, 8, 2, 3, 0, 8), (2, 41, 2, 1, 0, 8), (513, 8, 2, 1, 0, 8), (257, 8, 2, 2, 0, 8), (129, 9, 2, 3, 0, 8)):
        assert _lib.lib.zk_pcs_proof_bytes(*bad, c.byref(n)) == BAD, bad
    assert _lib.lib.zk_pcs_proof_bytes(2, 8, 2, 2, 0, 8, None) == BAD and n.value == 77


@pytest.mark.parametrize("k", (1, 2, 5))
def test_both_verifiers_accept_every_honest_proof(proofs, k):
    for case in (cs for cs in ref.CASES if cs[0] == k):
        field, _, shift, seed, z, root, ys, proof = proofs[case]
        assert len(proof) == ref.proof_bytes(*case)
        assert _both(field, case, shift, seed, root, z, ys, proof), case
    case = [cs for cs in ref.CASES if cs[0] == k][-1]
    field, _, shift, seed, z, root, ys, proof = proofs[case]
    assert zk_amd.pcs_verify(field, root, orc.from_int(field, z), orc.from_ints(field, ys), proof, *case[1:], orc.from_int(field, shift), seed)


@pytest.mark.parametrize("k", (1, 2, 5))
def test_both_verifiers_reject_every_kind_of_change(proofs, k):
    """per case: one y_c, z, the root, one element of a queried commitment row, one path digest, one entry of a round-0 FRI row, an element
    set to p, a wrong length.  The library on every case; the definition beside it (identical verdicts) on every third."""
    rng = random.Random(0x9C5B + k)
    for n, case in enumerate(cs for cs in ref.CASES if cs[0] == k):
        field, _, shift, seed, z, root, ys, proof = proofs[case]
        p = orc.modulus(field)
        _, d, b, a, f, q = case
        rounds, width, log_m = (d - f) // a, k << a, d + b - a
        fri_len = fri_ref.proof_bytes(d, b, a, f, q)
        per_open = 32 * (width + log_m)
        t = rng.randrange(q)
        row_at = fri_len + t * per_open + 32 * rng.randrange(width)
        path_at = fri_len + t * per_open + 32 * width + 32 * rng.randrange(log_m)
        r0_at = 32 * (rounds + (1 << f)) + t * (fri_len - 32 * (rounds + (1 << f))) // q + 32 * rng.randrange(1 << a)
        ys_bad = list(ys)
        ys_bad[rng.randrange(k)] = (ys_bad[rng.randrange(k)] + 1 + rng.randrange(p - 1)) % p
        if ys_bad == list(ys):
            ys_bad[0] = (ys[0] + 1) % p
        z_bad = (z + 1) % p
        while ref.on_domain(field, d + b, shift, z_bad):
            z_bad = (z_bad + 1) % p
        flipped_root = bytes([root[0] ^ 1]) + root[1:]
        changes = {
            "value": (root, z, ys_bad, proof),
            "z": (root, z_bad, ys, proof),
            "root": (flipped_root, z, ys, proof),
            "row_element": (root, z, ys, _put(proof, row_at, (int.from_bytes(proof[row_at:row_at + 32], "big") + 1) % p)),
            "path_digest": (root, z, ys, proof[:path_at + 7] + bytes([proof[path_at + 7] ^ 0x10]) + proof[path_at + 8:]),
            "fri_round0_entry": (root, z, ys, _put(proof, r0_at, (int.from_bytes(proof[r0_at:r0_at + 32], "big") + 1) % p)),
            "row_element_is_p": (root, z, ys, _put(proof, row_at, p)),
            "fri_round0_entry_is_p": (root, z, ys, _put(proof, r0_at, p)),
        }
        for name, (rt, zz, yy, pf) in changes.items():
            assert _verify_raw(field, case, shift, seed, rt, zz, yy, pf) == (0, 0), (case, name)
            if n % 3 == 0:
                assert not ref.verify(field, *case, shift, seed, rt, zz, yy, pf), (case, name)
        for bad_len in (proof[:-1], proof[:-32], proof + bytes(32)):
            assert _verify_raw(field, case, shift, seed, root, z, ys, bad_len)[0] == BAD, case      # a wrong length is refused outright
            assert not ref.verify(field, *case, shift, seed, root, z, ys, bad_len), case
        assert _verify_raw(field, case, shift, seed, root, z, ys, proof) == (0, 1), case


@pytest.mark.parametrize("extra", (1, 2), ids=("one_coefficient_over", "two_coefficients_over"))
@pytest.mark.parametrize("fi", range(3), ids=fri_ref.FIELD_IDS)
def test_a_polynomial_over_the_degree_bound_is_rejected(fi, extra):
    """a proof made from a polynomial with 2^d + extra coefficients, LDE'd at d + b, against the claim of its TRUE value.  Seeds are tried in
    order until the definition rejects (Q = 8: almost always the first); the library gives the definition's verdict on every one.

    extra = 1 is why FRI runs on X q(X) and not on q: f has 2^d + 1 coefficients, so q = (f - f(z)) / (X - z) has exactly 2^d, FRI's own
    bound, and a proof of q alone would be honest and complete.  X q(X) has 2^d + 1 and is rejected; an honest q has at most 2^d - 1 and
    X q(X) stays inside the bound (the accepted proofs of the tests above)."""
    p = orc.modulus(fi)
    rng = random.Random(0xB0D + fi)
    rejected = 0
    for case in ((1, 3, 1, 1, 0, 8), (2, 4, 2, 2, 0, 8), (5, 6, 1, 3, 0, 8), (2, 5, 2, 1, 1, 8), (1, 7, 1, 2, 1, 8)):
        k, d, b, a, f, q = case
        shift = (5, p - 1, 1)[fi]
        polys = [[rng.randrange(1, p) for _ in range((1 << d) + (extra if cc == k - 1 else 0))] for cc in range(k)]
        z = rng.randrange(p)
        while ref.on_domain(fi, d + b, shift, z):
            z = rng.randrange(p)
        root = ref.merkle_ref.root(ref.commit(fi, polys, d, b, a, shift)[2])
        for n in range(64):
            seed = bytes([fi, n, k, d, b, a]) + bytes(26)
            ys, proof = ref.prove(fi, polys, d, b, a, f, q, shift, seed, z)
            assert ys == [ref.evaluate(fi, co, z) for co in polys]
            if not _both(fi, case, shift, seed, root, z, ys, proof):
                rejected += 1
                break
        else:
            raise AssertionError(f"no seed of 64 makes the definition reject {case}")
        honest = [co[:1 << d] for co in polys]
        ys, proof = ref.prove(fi, honest, d, b, a, f, q, shift, bytes(32), z)
        assert _both(fi, case, shift, bytes(32), ref.merkle_ref.root(ref.commit(fi, honest, d, b, a, shift)[2]), z, ys, proof)
    assert rejected == 5


def test_verify_host_argument_table(proofs):
    lib = _lib.lib
    case = (2, 4, 1, 2, 0, 1)
    field, _, shift, seed, z, root, ys, proof = proofs[case]
    p = orc.modulus(field)
    k, d, b, a, f, q = case
    ok = c.c_int32(-7)
    sv, zv, yv = orc.from_int(field, shift), orc.from_int(field, z), np.ascontiguousarray(orc.from_ints(field, ys))
    sd, rt, pv = _u8(seed), _u8(root), _u8(proof)
    sp, zp, yp = (x.ctypes.data_as(_lib.u64p) for x in (sv, zv, yv))
    dp, rp, pp = (x.ctypes.data_as(_lib.u8p) for x in (sd, rt, pv))
    n = len(proof)
    assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, sp, dp, rp, zp, yp, pp, n, c.byref(ok)) == 0 and ok.value == 1
    ok.value = -7
    for i in range(6):   # every NULL pointer
        args = [sp, dp, rp, zp, yp, pp]
        args[i] = None
        assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, *args, n, c.byref(ok)) == BAD, i
    assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, sp, dp, rp, zp, yp, pp, n, None) == BAD
    assert lib.zk_pcs_verify_host(9, k, d, b, a, f, q, None, dp, rp, zp, yp, pp, n, c.byref(ok)) == BAD        # the NULL is seen first
    assert lib.zk_pcs_verify_host(9, k, d, b, a, f, q, sp, dp, rp, zp, yp, pp, n, c.byref(ok)) == BAD_FIELD
    assert lib.zk_pcs_verify_host(9, k, d, b, 0, f, q, sp, dp, rp, zp, yp, pp, n, c.byref(ok)) == BAD_FIELD    # the field before the parameters
    for bad in ((0, d, b, a, f, q), (k, d, b, 0, f, q), (k, d, b, 4, f, q), (k, d, 0, a, f, q), (k, d, 9, a, f, q), (k, d, b, a, f, 0), (k, d, b, a, f, 1025),
                (k, d, b, a, d, q), (k, d, b, 3, f, q), (k, 41, b, 1, f, q), (257, d, b, a, f, q), (513, d, b, 1, f, q)):
        assert lib.zk_pcs_verify_host(field, *bad, sp, dp, rp, zp, yp, pp, n, c.byref(ok)) == BAD, bad
    # unreduced inputs: the shift (zero too), z and a value -- zero, the modulus itself and all ones
    for v in (0, p, (1 << 256) - 1):
        raw = _raw(v).ctypes.data_as(_lib.u64p)
        assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, raw, dp, rp, zp, yp, pp, n, c.byref(ok)) == BAD, v
        if v:
            assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, sp, dp, rp, raw, yp, pp, n, c.byref(ok)) == BAD, v
            vals = np.ascontiguousarray(np.stack([yv[0], _raw(v)]))
            assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, sp, dp, rp, zp, vals.ctypes.data_as(_lib.u64p), pp, n, c.byref(ok)) == BAD, v
    # z on the domain: s w^5, and s itself
    for e in (5, 0):
        on = orc.from_int(field, shift * pow(fri_ref.root(field, 1 << (d + b)), e, p) % p)
        assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, sp, dp, rp, on.ctypes.data_as(_lib.u64p), yp, pp, n, c.byref(ok)) == BAD, e
    assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, sp, dp, rp, zp, yp, pp, n - 1, c.byref(ok)) == BAD
    assert lib.zk_pcs_verify_host(field, k, d, b, a, f, q, sp, dp, rp, zp, yp, pp, n + 32, c.byref(ok)) == BAD
    big = (1, 27, 2, 3, 0, 1)   # a domain past BN254's two-adicity (2^28): the length is looked at first, so it has to fit
    one = orc.from_int(0, 1)
    five = orc.from_int(0, 5)
    assert lib.zk_pcs_verify_host(0, *big, five.ctypes.data_as(_lib.u64p), dp, rp, one.ctypes.data_as(_lib.u64p), one.ctypes.data_as(_lib.u64p), pp,
                                  ref.proof_bytes(*big), c.byref(ok)) == NO_ROOT
    assert ok.value == -7   # nothing was written by any of them
    with pytest.raises(ZkError):
        zk_amd.pcs_verify(field, root, zv, yv, proof, d, b, a, f, q, sv, seed[:-1])


def test_device_calls_reject_bad_arguments_without_gpu():
    lib = _lib.lib
    fake = c.c_void_p(8)   # never dereferenced: a NULL among the others ends the call first
    h, ms, n = c.c_void_p(), c.c_double(-1.0), c.c_uint32(77)
    one = np.ones(4, dtype=np.uint64)
    ep = one.ctypes.data_as(_lib.u64p)
    buf = np.zeros(64, dtype=np.uint8)
    bp = buf.ctypes.data_as(_lib.u8p)
    arr = (c.c_void_p * 2)(8, 8)
    cols = c.cast(arr, _lib.vpp)
    holes = c.cast((c.c_void_p * 2)(8, None), _lib.vpp)
    q = lib.zk_deep_quotient
    assert q(None, cols, 2, ep, ep, ep, ep, fake) == BAD and q(fake, None, 2, ep, ep, ep, ep, fake) == BAD and q(fake, cols, 0, ep, ep, ep, ep, fake) == BAD
    assert q(fake, cols, 2, None, ep, ep, ep, fake) == BAD and q(fake, cols, 2, ep, None, ep, ep, fake) == BAD and q(fake, cols, 2, ep, ep, None, ep, fake) == BAD
    assert q(fake, cols, 2, ep, ep, ep, None, fake) == BAD and q(fake, cols, 2, ep, ep, ep, ep, None) == BAD and q(fake, holes, 2, ep, ep, ep, ep, fake) == BAD
    cm = lib.zk_pcs_commit
    assert cm(None, cols, 2, 4, 1, 2, ep, c.byref(h)) == BAD and cm(fake, None, 2, 4, 1, 2, ep, c.byref(h)) == BAD and cm(fake, cols, 0, 4, 1, 2, ep, c.byref(h)) == BAD
    assert cm(fake, cols, 2, 4, 1, 2, None, c.byref(h)) == BAD and cm(fake, cols, 2, 4, 1, 2, ep, None) == BAD and cm(fake, holes, 2, 4, 1, 2, ep, c.byref(h)) == BAD
    op = lib.zk_pcs_open
    assert op(None, fake, ep, 0, 1, bp, ep, bp) == BAD and op(fake, None, ep, 0, 1, bp, ep, bp) == BAD and op(fake, fake, None, 0, 1, bp, ep, bp) == BAD
    assert op(fake, fake, ep, 0, 1, None, ep, bp) == BAD and op(fake, fake, ep, 0, 1, bp, None, bp) == BAD and op(fake, fake, ep, 0, 1, bp, ep, None) == BAD
    assert lib.zk_pcs_root(None, fake, bp) == BAD and lib.zk_pcs_root(fake, None, bp) == BAD and lib.zk_pcs_root(fake, fake, None) == BAD
    assert lib.zk_pcs_n_polys(None, c.byref(n)) == BAD and lib.zk_pcs_n_polys(fake, None) == BAD
    assert lib.zk_pcs_free(None) == 0
    bq = lib.zk_bench_deep_quotient
    assert bq(None, cols, 2, fake, 1, c.byref(ms)) == BAD and bq(fake, None, 2, fake, 1, c.byref(ms)) == BAD and bq(fake, cols, 0, fake, 1, c.byref(ms)) == BAD
    assert bq(fake, cols, 2, None, 1, c.byref(ms)) == BAD and bq(fake, cols, 2, fake, 0, c.byref(ms)) == BAD and bq(fake, cols, 2, fake, 1, None) == BAD
    assert h.value is None and ms.value == -1.0 and n.value == 77 and not buf.any()


def test_commit_without_gpu_fails_loudly():
    if not _no_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ZkError) as e:
        ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
        zk_amd.PolyCommitment.commit([zk_amd.UnivariatePolynomial.new(ctx, np.zeros((2, 4), dtype=np.uint64))], 1, 1, 1, orc.from_int(0, 5))
    assert e.value.code == -22 and "no CPU fallback" in str(e.value)   # ZK_ERR_NO_DEVICE's message, not a fallback


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_pcs")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_pcs.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    if not _no_gpu():
        pytest.skip("GPU present: run by tests/test_gpu_pcs.py")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr
