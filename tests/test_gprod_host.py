"""The definition of the grand-product argument (tests/gprod_ref.py) checked on its own, and the host verifier zk_gprod_verify_host against
it on the shared case list: every honest proof accepted by both with equal point and claim, every kind of change rejected by both with
equal verdicts, a cheating prover, zk_gprod_proof_bytes, the argument table, the tree kernels' constants, the new exports and their
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
import gprod_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, BAD_FIELD = -20, -21
SYMBOLS = ("zk_mle_product_tree", "zk_gprod_proof_bytes", "zk_gprod_prove", "zk_gprod_verify_host", "zk_bench_gprod")
WRAPPERS = ("product_tree", "grand_product_prove", "grand_product_verify", "grand_product_verify_table", "gprod_proof_bytes", "bench_gprod")
UNTOUCHED = 0x0909090909090909


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _raw(v):
    """limbs of an integer as they are, reduced or not"""
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def _verify_raw(field, n, shift, seed, product, proof, proof_len=None, raw_shift=None, raw_product=None):
    """(status, ok, point, claim) of zk_gprod_verify_host on raw buffers; shift (None = NULL), product: canonical ints; point and claim
    as ints when the proof was accepted, else whether the buffers were left alone"""
    ok = c.c_int32(-7)
    sv = raw_shift if raw_shift is not None else (None if shift is None else orc.from_int(field, shift))
    pv = raw_product if raw_product is not None else orc.from_int(field, product)
    point, claim = np.full((41, 4), UNTOUCHED, dtype=np.uint64), np.full(4, UNTOUCHED, dtype=np.uint64)
    sd, pf = _u8(seed), _u8(proof)
    rc = _lib.lib.zk_gprod_verify_host(field, n, None if sv is None else sv.ctypes.data_as(_lib.u64p), sd.ctypes.data_as(_lib.u8p),
                                       pv.ctypes.data_as(_lib.u64p), pf.ctypes.data_as(_lib.u8p), len(proof) if proof_len is None else proof_len,
                                       point.ctypes.data_as(_lib.u64p), claim.ctypes.data_as(_lib.u64p), c.byref(ok))
    if rc == 0 and ok.value == 1:
        assert (point[n:] == UNTOUCHED).all()
        return rc, 1, orc.to_ints(field, point[:n]), orc.to_int(field, claim)
    return rc, ok.value, bool((point == UNTOUCHED).all()), bool((claim == UNTOUCHED).all())


def _both(field, n, shift, seed, product, proof):
    """the verdict of the library and of the definition, which must be the same (with equal point and claim on acceptance)"""
    rc, ok, point, claim = _verify_raw(field, n, shift, seed, product, proof)
    want = ref.verify(field, n, seed, product, proof, shift)
    assert rc == 0 and ok == int(want is not None), (n, rc, ok, want)
    if want is None:
        assert point is True and claim is True   # nothing was written
        return None
    assert (point, claim) == (list(want[0]), want[1])
    return want


def _put(proof, at, value):
    return proof[:at] + int(value).to_bytes(32, "big") + proof[at + 32:]


@pytest.fixture(scope="module")
def proofs():
    """{case: (field, table, shift, seed, P, proof, point, claim)} for the shared case list from the definition, computed once"""
    out = {}
    for case in ref.CASES:
        field, table, shift, seed = ref.case_inputs(case, worst_case_values)
        out[case] = (field, table, shift, seed) + ref.prove(field, table, seed, shift)
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
    assert re.search(r"^OBJS := .*\bgprod\.o\b", make, flags=re.M)
    assert 'env_u64("ZK_GPROD_TREE_FUSE"' in open(os.path.join(ROOT, "zk_amd", "csrc", "gprod.hip")).read()


def test_case_lists_and_kernel_constants():
    assert sorted(cs[0] for cs in ref.CASES if not cs[2]) == sorted(list(range(1, 9)) * 2)
    assert {cs[2] for cs in ref.CASES} == {"", "zero", "cancel"}
    assert {ref.case_field(cs) for cs in ref.CASES} == {0, 1, 2}
    assert {ref.case_shift_kind(cs) for cs in ref.CASES} == set(ref.SHIFT_KINDS)
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "gprod_kernels.cuh")).read()
    common = open(os.path.join(ROOT, "zk_amd", "csrc", "common.cuh")).read()
    core = open(os.path.join(ROOT, "zk_amd", "csrc", "host_core.hpp")).read()
    assert ref.THREADS == int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    assert ref.LDS_VARS == int(re.search(r"constexpr uint32_t kPtreeLdsVars = (\d+);", src).group(1))
    assert ref.FUSE_MAX == int(re.search(r"constexpr uint32_t kPtreeMaxFuse = (\d+);", src).group(1))
    assert ref.FUSE_DEFAULT == int(re.search(r"constexpr uint32_t kPtreeFuseDefault = (\d+);", src).group(1))
    assert ref.MAX_BLOCKS_STREAM == int(re.search(r"constexpr uint32_t kMaxGridStream = (\d+);", core).group(1))
    assert ref.MAX_VARS == int(re.search(r"constexpr uint64_t kMaxVars = (\d+);", core).group(1))
    L = ref.LDS_VARS
    # a fused launch's lowest level is a whole number of workgroups of whole 64-element runs
    assert (1 << L) % ref.THREADS == 0 and ref.THREADS % 64 == 0
    assert ref.launches(L) == [] and ref.launches(1) == []
    assert [ref.launches(L + k) for k in (1, 2, 3, 4)] == [[(1, L)], [(2, L)], [(3, L)], [(3, L + 1), (1, L)]]
    assert ref.launches(L + 3, 1) == [(1, L + 2), (1, L + 1), (1, L)] and ref.launches(L + 3, 2) == [(2, L + 1), (1, L)]
    # the extras: 0, 1, 2 levels mod 3 above the LDS stage, one that needs two fused launches, all three fields, nothing above 2^14
    extra = ref.GPU_EXTRA_CASES
    assert {(cs[0] - L) % 3 for cs in extra} == {0, 1, 2} and any(len(ref.launches(cs[0])) == 2 for cs in extra)
    assert {ref.case_field(cs) for cs in extra} == {0, 1, 2} and max(cs[0] for cs in extra) <= 14
    assert ref.TREE_VARS == tuple(range(1, L + 3))
    # the capped grid: 2^14 workgroups of 256 threads take one element each up to a lowest level of 2^22
    assert ref.SECOND_TRIP_VARS == {1: 24, 2: 25, 3: 26}
    assert ref.trips(25) == 1 and ref.trips(26) == 2 and ref.trips(23, 1) == 1 and ref.trips(24, 1) == 2
    assert ref.SECOND_TRIP_VARS[ref.FUSE_DEFAULT] > 25   # the default route never loops below 2^25 elements


def test_the_tree_is_the_product():
    for case in ref.CASES:
        field, table, shift, seed = ref.case_inputs(case, worst_case_values)
        p = orc.modulus(field)
        n = case[0]
        want = 1
        for x in table:
            want = want * (x + (shift or 0)) % p
        levels = ref.tree(table, shift, p)
        heap = ref.product_tree(table, shift, p)
        assert levels[0] == [want] and len(levels) == n + 1 and len(heap) == 1 << n and heap[0] == 1 and heap[1] == want
        for j in range(n):
            assert heap[1 << j:2 << j] == levels[j]
            # a node is the product of the leaves under it: those that agree with it in the LOW j index bits
            for i in (0, (1 << j) - 1):
                sub = 1
                for k in range(i, 1 << n, 1 << j):
                    sub = sub * (table[k] + (shift or 0)) % p
                assert levels[j][i] == sub
        if case[2]:
            assert want == 0 and ((0 in table) if case[2] == "zero" else ((p - shift) % p in table and 0 not in table))
        else:
            assert want != 0


def test_completeness_and_proof_bytes(proofs):
    for case, (field, table, shift, seed, product, proof, point, claim) in proofs.items():
        n = case[0]
        p = orc.modulus(field)
        assert product == ref.tree(table, shift, p)[0][0]
        got = ref.verify(field, n, seed, product, proof, shift)
        assert got == (point, claim) and len(point) == n, case
        assert ref.evaluate(table, point, p) == claim, case            # the claim the verifier is left with is true
        assert _both(field, n, shift, seed, product, proof) is not None, case
        assert len(proof) == ref.proof_bytes(n) == zk_amd.gprod_proof_bytes(n) == 64 * n * n, case
        out = zk_amd.grand_product_verify(field, n, seed, orc.from_int(field, product), proof, None if shift is None else orc.from_int(field, shift))
        assert out is not None and orc.to_ints(field, out[0]) == point and orc.to_int(field, out[1]) == claim


def test_null_and_zero_shift_give_the_same_bytes(proofs):
    for case, (field, table, shift, seed, product, proof, point, claim) in proofs.items():
        if shift in (None, 0):
            for other in (None, 0):
                assert ref.prove(field, table, seed, other) == (product, proof, point, claim)
                assert _both(field, case[0], other, seed, product, proof) == (point, claim)
    assert {None, 0} <= {v[2] for v in proofs.values()}


def test_every_change_is_rejected_by_both(proofs):
    for case, (field, table, shift, seed, product, proof, point, claim) in proofs.items():
        n = case[0]
        p = orc.modulus(field)
        assert _both(field, n, shift, seed, (product + 1) % p, proof) is None, case
        # another seed or shift is another tau_0: from n = 2 on layer 1's first round check fails; at n = 1 there is no later check (a b = P
        # holds) and what changes is the point and the claim that are handed out
        for got in (_both(field, n, shift, bytes([seed[0] ^ 1]) + seed[1:], product, proof), _both(field, n, ((shift or 0) + 1) % p, seed, product, proof)):
            assert (got is None) if n >= 2 else (got is not None and got[0] != point and got[1] != claim), case
        if n >= 3:   # one element changed in each section: layer 0's pair, a round evaluation of the first and of the last layer, an a, a b
            for name, at in ref.section_offsets(n).items():
                bad = bytearray(proof)
                bad[at + 31] ^= 1
                assert _both(field, n, shift, seed, product, bytes(bad)) is None, (case, name)
                assert _both(field, n, shift, seed, product, _put(proof, at, p)) is None, (case, name)   # an element >= p
        else:
            for at in range(0, len(proof), 32):
                bad = bytearray(proof)
                bad[at + 31] ^= 1
                assert _both(field, n, shift, seed, product, bytes(bad)) is None, (case, at)
        # the same bytes under another n: another length, which the definition rejects and the library refuses
        for other in (proof[:-1], proof + b"\0", proof[:-32], proof + proof[-32:]):
            assert ref.verify(field, n, seed, product, other, shift) is None
            assert _verify_raw(field, n, shift, seed, product, other) == (BAD, -7, True, True)
        for m in (n - 1, n + 1):
            if m >= 1:
                assert ref.verify(field, m, seed, product, proof, shift) is None
                assert _verify_raw(field, m, shift, seed, product, proof) == (BAD, -7, True, True)
        # ... and padded to that n's length, so that the transcript's n is what rejects it
        padded = (proof + bytes(64 * (n + 1) * (n + 1)))[:64 * (n + 1) * (n + 1)]
        assert _both(field, n + 1, shift, seed, product, padded) is None, case


def test_a_cheating_prover_is_rejected(proofs):
    """the sumchecks are run on a tree with one inner node changed (so the claimed product, or a layer's link, is false): deterministic
    under the fixed seeds, and rejected by both"""
    for case in [cs for cs in ref.CASES if cs[0] >= 2]:
        field, table, shift, seed = proofs[case][:4]
        n = case[0]
        p = orc.modulus(field)
        for j in sorted({0, n // 2, n - 1}):   # the root itself, a middle level, the level under the leaves' products
            levels = [list(level) for level in ref.tree(table, shift, p)]
            levels[j][(1 << j) - 1] = (levels[j][(1 << j) - 1] + 1) % p
            product, proof, point, claim = ref.prove(field, table, seed, shift, levels=levels)
            assert _both(field, n, shift, seed, product, proof) is None, (case, j)
        # changed leaves are another table: the argument goes through, and the claim left over is false for t
        levels = [list(level) for level in ref.tree(table, shift, p)]
        levels[n][0] = (levels[n][0] + 1) % p
        for j in range(n - 1, -1, -1):
            levels[j] = [levels[j + 1][i] * levels[j + 1][i + (1 << j)] % p for i in range(1 << j)]
        product, proof, point, claim = ref.prove(field, table, seed, shift, levels=levels)
        assert _both(field, n, shift, seed, product, proof) == (point, claim)
        assert ref.evaluate(table, point, p) != claim, case


def test_argument_table(proofs):
    case = (4, 0, "")
    field, table, shift, seed, product, proof, point, claim = proofs[case]
    n = 4
    p = orc.modulus(field)
    u64p, u8p = _lib.u64p, _lib.u8p
    assert _verify_raw(field, n, shift, seed, product, proof)[:2] == (0, 1)
    sd, pf, pv = _u8(seed), _u8(proof), orc.from_int(field, product)
    pt, cl, ok = np.full((n, 4), UNTOUCHED, dtype=np.uint64), np.full(4, UNTOUCHED, dtype=np.uint64), c.c_int32(-7)
    args = [field, n, None, sd.ctypes.data_as(u8p), pv.ctypes.data_as(u64p), pf.ctypes.data_as(u8p), len(proof), pt.ctypes.data_as(u64p),
            cl.ctypes.data_as(u64p), c.byref(ok)]
    for i in (3, 4, 5, 7, 8, 9):   # every pointer but the shift
        bad = list(args)
        bad[i] = None
        assert _lib.lib.zk_gprod_verify_host(*bad) == BAD, i
    # a NULL with an unknown field: the NULL is reported; an unknown field before a bad n
    assert _lib.lib.zk_gprod_verify_host(7, n, None, None, *args[4:]) == BAD
    assert _lib.lib.zk_gprod_verify_host(7, 0, *args[2:]) == BAD_FIELD
    assert (pt == UNTOUCHED).all() and (cl == UNTOUCHED).all() and ok.value == -7
    for bad_n in (0, 41):
        assert _verify_raw(field, bad_n, shift, seed, product, proof) == (BAD, -7, True, True)
    assert _verify_raw(field, n, shift, seed, product, proof, raw_shift=_raw(p)) == (BAD, -7, True, True)
    assert _verify_raw(field, n, shift, seed, product, proof, raw_product=_raw(p)) == (BAD, -7, True, True)
    assert _verify_raw(field, n, shift, seed, product, proof, raw_product=_raw((1 << 256) - 1)) == (BAD, -7, True, True)
    assert _verify_raw(field, n, shift, seed, product, proof, proof_len=len(proof) - 32) == (BAD, -7, True, True)
    out = c.c_uint64(5)
    for bad_n in (0, 41, 1 << 31):
        assert _lib.lib.zk_gprod_proof_bytes(bad_n, c.byref(out)) == BAD and out.value == 5
    assert _lib.lib.zk_gprod_proof_bytes(4, None) == BAD
    assert _lib.lib.zk_gprod_proof_bytes(40, c.byref(out)) == 0 and out.value == 64 * 1600
