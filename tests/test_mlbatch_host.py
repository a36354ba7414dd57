"""The definition of the batch multilinear commitment (tests/mlbatch_ref.py) checked on its own, and the host verifier
zk_mlbatch_verify_host against it on the shared case list: every honest proof accepted by both, every kind of change rejected by both with
equal verdicts, three cheating provers, the exact-length rule, unreduced elements, random bytes, zk_mlbatch_proof_bytes and the proof-size
statement, the k = 1 root, the sumcheck algebra of the per-point device sums in plain integers, the kernels' constants, the new exports
and their Python signatures -- all without a GPU.  Everything is bytes."""
import ctypes as c
import os
import random
import re
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_ref  # noqa: E402
import mlbatch_ref as ref  # noqa: E402
import mlpcs_ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ROOT, BAD, BAD_FIELD = -7, -20, -21
SYMBOLS = ("zk_mlbatch_commit", "zk_mlbatch_free", "zk_mlbatch_n_vars", "zk_mlbatch_n_tables", "zk_mlbatch_root", "zk_mlbatch_proof_bytes",
           "zk_mlbatch_open", "zk_mlbatch_verify_host", "zk_mle_lincomb", "zk_mle_eq_sums_many", "zk_bench_mlbatch")
WRAPPERS = ("MultilinearBatchCommitment", "mlbatch_verify", "mlbatch_proof_bytes", "lincomb", "eq_sums_many", "bench_mlbatch")


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _raw(v):
    """limbs of an integer as they are, reduced or not"""
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def _verify_raw(field, case, shift, seed, root, points, values, proof, proof_len=None, raw_points=None, raw_values=None, raw_shift=None,
                call_field=None):
    """(status, ok) of zk_mlbatch_verify_host on raw buffers; shift, points, values: canonical ints"""
    n, b, f, q, k, m = case
    ok = c.c_int32(-7)
    sv = orc.from_int(field, shift) if raw_shift is None else raw_shift
    zv = np.ascontiguousarray(orc.from_ints(field, [x for z in points for x in z])) if raw_points is None else raw_points
    vv = np.ascontiguousarray(orc.from_ints(field, [x for row in values for x in row])) if raw_values is None else raw_values
    sd, rt, pv = _u8(seed), _u8(root), _u8(proof)
    rc = _lib.lib.zk_mlbatch_verify_host(field if call_field is None else call_field, n, k, m, b, f, q, sv.ctypes.data_as(_lib.u64p),
                                         sd.ctypes.data_as(_lib.u8p), rt.ctypes.data_as(_lib.u8p), zv.ctypes.data_as(_lib.u64p),
                                         vv.ctypes.data_as(_lib.u64p), pv.ctypes.data_as(_lib.u8p), len(proof) if proof_len is None else proof_len,
                                         c.byref(ok))
    return rc, ok.value


def _both(field, case, shift, seed, root, points, values, proof):
    """the verdict of the library and of the definition, which must be the same"""
    n, b, f, q, k, m = case
    rc, ok = _verify_raw(field, case, shift, seed, root, points, values, proof)
    want = ref.verify(field, n, b, f, q, k, shift, seed, root, points, values, proof)
    assert rc == 0 and ok == int(want), (case, rc, ok, want)
    return want


def _put(proof, at, value):
    return proof[:at] + int(value).to_bytes(32, "big") + proof[at + 32:]


@pytest.fixture(scope="module")
def proofs():
    """{case: (field, tables, shift, seed, points, committed, root, values, the definition's proof)} for the shared case list, computed once"""
    out = {}
    for case in ref.CASES:
        n, b, f, q, k, m = case
        field = ref.case_field(case)
        tables, shift, seed, points = ref.case_inputs(field, case, worst_case_values)
        committed = ref.commit(field, tables, b, shift)
        values, proof = ref.prove(field, tables, b, f, q, shift, seed, points, committed=committed)
        out[case] = (field, tables, shift, seed, points, committed, ref.merkle_ref.root(committed[2]), values, proof)
    return out


def test_exports_signatures_and_sources():
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(_lib.lib, name), name
        assert name in _lib._sig and name in _lib.declared_symbols(), name
        assert re.search(r"\bint32_t %s\(" % name, header), name
    for name in WRAPPERS:
        assert name in zk_amd.api.__all__ and hasattr(zk_amd, name), name
    make = open(os.path.join(ROOT, "zk_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS := .*\bmlbatch\.o\b", make, flags=re.M)
    unit = open(os.path.join(ROOT, "zk_amd", "csrc", "mlbatch.hip")).read()
    assert 'env_u64("ZK_MLBATCH_FUSE_FOLD"' in unit
    # the host helpers are shared through a header, not copied
    shared = open(os.path.join(ROOT, "zk_amd", "csrc", "ml_host.hpp")).read()
    for helper in ("ml_eq1", "ml_round_poly", "ml_quadratic_at", "ml_per_query"):
        assert re.search(r"^inline \w+ %s\(" % helper, shared, flags=re.M), helper
        for name in ("mlpcs.hip", "mlbatch.hip"):
            text = open(os.path.join(ROOT, "zk_amd", "csrc", name)).read()
            assert '#include "ml_host.hpp"' in text and not re.search(r"^(static|inline) \w+ %s\(" % helper, text, flags=re.M), (name, helper)


def test_case_lists_and_kernel_constants():
    full = {(n, b, f, q, k, m) for n in range(1, 9) for b in (1, 2) for f in (0, 2) for q in (1, 8) if f < n
            for k, m in ((1, 1), (2, 1), (3, 2), (5, ref.POINTS_PER_PASS + 1))}
    assert set(ref.ALL_CASES) == full and set(ref.CASES) <= full and len(set(ref.CASES)) == len(ref.CASES)
    # the thinning keeps every n, b, f, Q and (k, m), and all three fields
    for at, kinds in ((0, set(range(1, 9))), (1, {1, 2}), (2, {0, 2}), (3, {1, 8})):
        assert {cs[at] for cs in ref.CASES} == kinds, at
    assert {cs[4:] for cs in ref.CASES} == set(ref.KM) and {ref.case_field(cs) for cs in ref.CASES} == {0, 1, 2}
    assert any(cs[5] > ref.POINTS_PER_PASS and cs[0] - cs[2] >= 2 for cs in ref.CASES)       # sum-only passes behind a folding pass
    assert ref.EQUAL_POINTS_CASE in ref.CASES
    pts = ref.case_inputs(ref.case_field(ref.EQUAL_POINTS_CASE), ref.EQUAL_POINTS_CASE, worst_case_values)[3]
    assert pts[0] == pts[1]
    extras = {(11, 1, 2, 8, 3, 2), (12, 2, 0, 8, 2, ref.POINTS_PER_PASS + 1), (13, 1, 1, 1, 5, 1), (6, 1, 0, 8, 17, 1)}
    assert set(ref.GPU_CASES) == {cs for cs in ref.CASES if cs[3] == 8} | extras
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "mlbatch_kernels.cuh")).read()
    single = open(os.path.join(ROOT, "zk_amd", "csrc", "mlpcs_kernels.cuh")).read()
    unit = open(os.path.join(ROOT, "zk_amd", "csrc", "mlbatch.hip")).read()
    assert ref.POINTS_PER_PASS == int(re.search(r"constexpr uint32_t kMlPointsPerPass = (\d+);", src).group(1))
    assert ref.POINTS_PER_PASS & (ref.POINTS_PER_PASS - 1) == 0
    assert ref.LO_BITS == int(re.search(r"constexpr uint32_t kMlLoBits = (\d+);", single).group(1)) and '#include "mlpcs_kernels.cuh"' in src
    assert ref.LINCOMB_ELEMS_PER_THREAD == int(re.search(r"constexpr uint32_t kLincombPerThread = (\d+);", src).group(1))
    assert ref.LINCOMB_MAX_BLOCKS == int(re.search(r"constexpr uint32_t kLincombMaxGrid = (\d+);", src).group(1))
    assert (ref.MAX_TABLES, ref.MAX_POINTS) == tuple(int(x) for x in re.search(r"kMlBatchMaxTables = (\d+), kMlBatchMaxPoints = (\d+);", unit).groups())
    # the Lo tables of one pass and the wave sums fit the CU's LDS twice
    lds = ref.POINTS_PER_PASS * (32 << ref.LO_BITS) + 2 * ref.POINTS_PER_PASS * mlpcs_ref.WAVES_PER_BLOCK * 32
    assert 2 * lds <= 160 * 1024
    # the lincomb's launch shape: one trip up to 2^22 elements, the second from 2^23 on
    per_trip = ref.LINCOMB_MAX_BLOCKS * mlpcs_ref.THREADS * ref.LINCOMB_ELEMS_PER_THREAD
    n2 = ref.LINCOMB_SECOND_TRIP_VARS
    assert 1 << (n2 - 1) <= per_trip < 1 << n2 and ref.lincomb_trips(n2 - 1) == 1 and ref.lincomb_trips(n2) == 2 and n2 == 23
    assert set(ref.LINCOMB_VARS) == {0, 1, 5, 6, 7, 13} and set(ref.LINCOMB_COUNTS) == {1, 2, 3, 8}
    # (12, 2, 0, 8, 2, P + 1): layer 0 past the split of FRI's power table, rounds in every Hi / Lo regime, more points than a pass
    n, b, f, q, k, m = (12, 2, 0, 8, 2, ref.POINTS_PER_PASS + 1)
    ms = {n - 1 - r for r in range(1, n - f)}
    assert n + b > 12 and max(ms) > ref.LO_BITS and any(mlpcs_ref.RUN_MIN_BITS <= x < ref.LO_BITS for x in ms) and any(x < mlpcs_ref.RUN_MIN_BITS for x in ms)


def test_the_per_point_sums_give_the_round_polynomials():
    """the sumcheck side in plain integers: for T folded top bit first, the round polynomial made from the per-point sums S_X^j
    (round_from_sums: what the device leaves and the host combines) equals the direct sums of T E, round by round, and the last claim
    is sum_j c_R^j T_R(z_j[R:])"""
    for field, (n, k, m, f) in enumerate(((5, 3, 2, 0), (4, 2, ref.POINTS_PER_PASS + 1, 2), (3, 1, 1, 0))):
        p = fri_ref.modulus(field)
        rng = random.Random(90 + field)
        tables = ref.case_tables(p, field, n, k, worst_case_values)
        points = [[mlpcs_ref.point_entries(p, rng)[(i + j) % 4] for i in range(n)] for j in range(m)]
        lam, gam = rng.randrange(p), rng.randrange(p)
        t = ref.lincomb(tables, ref.powers(lam, k, p), p)
        e = ref.lincomb([mlpcs_ref.eq_table(z, p) for z in points], ref.powers(gam, m, p), p)
        scales = ref.powers(gam, m, p)
        claim = sum(scales[j] * sum(pow(lam, cc, p) * mlpcs_ref.evaluate(tables[cc], points[j], p) for cc in range(k)) for j in range(m)) % p
        for r in range(n - f):
            sums = ref.eq_sums_many(t, [z[r + 1:] for z in points], p)
            h = ref.round_from_sums(sums, scales, [z[r] for z in points], p)
            assert h == mlpcs_ref.round_sums(t, e, p), (field, r)
            assert (h[0] + h[1]) % p == claim, (field, r)
            beta = rng.randrange(p)
            claim = mlpcs_ref.quadratic_at(h, beta, p)
            t, e = mlpcs_ref.partial_evaluate0(t, beta, p), mlpcs_ref.partial_evaluate0(e, beta, p)
            scales = [sc * mlpcs_ref.eq1(beta, z[r], p) % p for sc, z in zip(scales, points)]
        assert claim == sum(sc * mlpcs_ref.evaluate(t, z[n - f:], p) for sc, z in zip(scales, points)) % p, field


def test_completeness_proof_bytes_and_size_statement(proofs):
    for case, (field, tables, shift, seed, points, committed, root, values, proof) in proofs.items():
        n, b, f, q, k, m = case
        p = fri_ref.modulus(field)
        assert values == [[mlpcs_ref.evaluate(t, z, p) for t in tables] for z in points]
        assert _both(field, case, shift, seed, root, points, values, proof) is True, case
        formula = 32 * (3 * (n - f) + (n - f) - 1 + 2 ** f) + 32 * q * ((2 * k + n + b - 1) + sum(2 + n + b - 1 - r for r in range(1, n - f)))
        assert len(proof) == formula == ref.proof_bytes(n, b, f, q, k, m) == zk_amd.mlbatch_proof_bytes(n, k, m, b, f, q), case
        if k * m >= 2:   # one batch proof is shorter than the k m separate openings it replaces
            assert len(proof) < k * m * mlpcs_ref.proof_bytes(n, b, f, q), case
        pv = np.stack([orc.from_ints(field, z) for z in points])
        vv = np.stack([orc.from_ints(field, row) for row in values])
        assert zk_amd.mlbatch_verify(field, root, pv, vv, proof, b, f, q, orc.from_int(field, shift), seed)
    kinds = {x for (field, tables, shift, seed, points, *_r) in proofs.values() for z in points for x in z}
    assert {0, 1} <= kinds and any(x == fri_ref.modulus(0) - 1 for x in kinds)
    assert any(cs[4] * cs[5] >= 2 for cs in proofs)


def test_the_root_of_one_table_is_the_single_commitment_s(proofs):
    for case, (field, tables, shift, seed, points, committed, root, values, proof) in proofs.items():
        if case[4] == 1:
            single = mlpcs_ref.commit(field, tables[0], case[1], shift)
            assert root == mlpcs_ref.merkle_ref.root(single[2]), case
    assert any(cs[4] == 1 for cs in proofs)


def test_every_change_is_rejected_by_both(proofs):
    for case, (field, tables, shift, seed, points, committed, root, values, proof) in proofs.items():
        n, b, f, q, k, m = case
        p = fri_ref.modulus(field)
        for j in range(m):                                   # one value
            for cc in {0, k - 1}:
                v2 = [list(row) for row in values]
                v2[j][cc] = (v2[j][cc] + 1) % p
                assert _both(field, case, shift, seed, root, points, v2, proof) is False, (case, j, cc)
        for j in {0, m - 1}:                                 # one coordinate of one point
            for i in range(n):
                z2 = [list(z) for z in points]
                z2[j][i] = (z2[j][i] + 1) % p
                assert _both(field, case, shift, seed, root, z2, values, proof) is False, (case, j, i)
        if k >= 2 and values[0][0] != values[0][1]:          # two tables' values swapped
            v2 = [list(row) for row in values]
            v2[0][0], v2[0][1] = v2[0][1], v2[0][0]
            assert _both(field, case, shift, seed, root, points, v2, proof) is False, case
        seed2 = bytes([seed[0] ^ 1]) + seed[1:]
        assert _both(field, case, shift, seed2, root, points, values, proof) is False, case
        # one byte flipped in each section: an h, a root, a final coefficient, a round-0 row element in an even and in an odd column, a
        # later row element, a path digest
        for name, at in ref.section_offsets(*case).items():
            if at is None:
                continue
            assert at + 32 <= len(proof), (case, name)
            bad = bytearray(proof)
            bad[at + 31] ^= 1
            assert _both(field, case, shift, seed, root, points, values, bytes(bad)) is False, (case, name)
            assert _both(field, case, shift, seed, root, points, values, _put(proof, at, p)) is False, (case, name)   # an element >= p
        # the exact-length rule: the definition rejects, the library refuses the length
        for other in (proof[:-1], proof + b"\0", proof[:-32], proof + proof[-32:]):
            assert not ref.verify(field, n, b, f, q, k, shift, seed, root, points, values, other)
            assert _verify_raw(field, case, shift, seed, root, points, values, other) == (BAD, -7)
        assert _verify_raw(field, case, shift, seed, root, points, values, proof, proof_len=len(proof) - 1) == (BAD, -7)
        assert _verify_raw(field, case, shift, seed, root, points, values, proof + b"\0", proof_len=len(proof) + 1) == (BAD, -7)
    offs = [ref.section_offsets(*cs) for cs in proofs]
    assert all(any(o[name] is not None for o in offs) for name in ("h", "root", "final", "row_even", "row_odd", "row_later", "path"))


def test_random_bytes_and_other_parameters_are_rejected(proofs):
    rng = random.Random(4)
    for case, (field, tables, shift, seed, points, committed, root, values, proof) in proofs.items():
        n, b, f, q, k, m = case
        junk = bytes(rng.randrange(256) for _ in range(len(proof)))
        assert _both(field, case, shift, seed, root, points, values, junk) is False, case
        # the same bytes under another k or m with the same length (m does not enter the length): the transcript's parameters reject them
        if m + 1 <= ref.MAX_POINTS:
            other = (n, b, f, q, k, m + 1)
            assert _both(field, other, shift, seed, root, points + [points[0]], values + [values[0]], proof) is False, case


def test_three_cheating_provers(proofs):
    """a prover whose sumcheck runs on another table c than the committed one; one whose committed codeword c is not the table's (the LDE
    of 2^n + 1 coefficients); one whose value matrix is wrong but consistent under lambda = 1 (two entries of a row offset by +d and -d):
    the verdicts are deterministic under the fixed seeds, and all three are rejected by both"""
    cases = [cs for cs in ref.CASES if cs[3] == 8 and cs[0] >= 2]
    assert any(cs[4] >= 2 for cs in cases)
    for case in cases:
        field, tables, shift, seed, points, committed, root, values, proof = proofs[case]
        n, b, f, q, k, m = case
        p = fri_ref.modulus(field)
        cc = k - 1
        # the changed entry: where eq(., z_0) does not vanish in the variables the final polynomial keeps (z_j = 1 -> bit 1, else bit 0);
        # the folded variables meet random betas
        z = points[0]
        at = sum((1 if (z[j] == 1 or (j < n - f and j % 2)) else 0) << (n - 1 - j) for j in range(n))
        other = [list(t) for t in tables]
        other[cc][at] = (other[cc][at] + 1) % p
        v2, proof2 = ref.prove(field, tables, b, f, q, shift, seed, points, sumcheck_tables=other, committed=committed)
        assert v2[0][cc] == mlpcs_ref.evaluate(other[cc], z, p) and [row[:cc] for row in v2] == [row[:cc] for row in values]
        assert _both(field, case, shift, seed, root, points, v2, proof2) is False, case
        coeffs = ref.cmle_ref.interpolate_fast(list(tables[cc]), p)[1] + [1 + n]   # one coefficient past the bound
        com3 = ref.commit(field, tables, b, shift, layer0s={cc: fri_ref.lde(field, coeffs, n + b, shift)})
        v3, proof3 = ref.prove(field, tables, b, f, q, shift, seed, points, committed=com3)
        assert v3 == values
        assert _both(field, case, shift, seed, ref.merkle_ref.root(com3[2]), points, v3, proof3) is False, case
        if k >= 2:
            v4 = [list(row) for row in values]
            v4[m - 1][0], v4[m - 1][1] = (v4[m - 1][0] + 5) % p, (v4[m - 1][1] - 5) % p
            assert sum(v4[m - 1]) % p == sum(values[m - 1]) % p
            got, proof4 = ref.prove(field, tables, b, f, q, shift, seed, points, values=v4, committed=committed)
            assert got == v4
            assert _both(field, case, shift, seed, root, points, v4, proof4) is False, case


def test_argument_table(proofs):
    case = next(cs for cs in ref.CASES if cs[4] >= 2 and cs[5] >= 2 and cs[0] >= 4)
    field, tables, shift, seed, points, committed, root, values, proof = proofs[case]
    n, b, f, q, k, m = case
    p = fri_ref.modulus(field)
    assert _verify_raw(field, case, shift, seed, root, points, values, proof) == (0, 1)
    assert _verify_raw(field, case, shift, seed, root, points, values, proof, call_field=7) == (BAD_FIELD, -7)
    big_points = [list(z) + [0] * 40 for z in points] + [[0] * 60] * 20
    big_values = [list(row) + [0] * 300 for row in values] + [[0] * 300] * 20
    for bad in ((0, b, 0, q, k, m), (n, 0, f, q, k, m), (n, 9, f, q, k, m), (n, b, n, q, k, m), (n, b, f, 0, k, m), (n, b, f, 1025, k, m),
                (41, b, f, q, k, m), (n, b, f, q, 0, m), (n, b, f, q, 257, m), (n, b, f, q, k, 0), (n, b, f, q, k, 17)):
        zs = [z[:max(bad[0], 1)] for z in big_points[:max(bad[5], 1)]]
        vs = [row[:max(bad[4], 1)] for row in big_values[:max(bad[5], 1)]]
        assert _verify_raw(field, bad, shift, seed, root, zs, vs, proof) == (BAD, -7), bad
    assert _verify_raw(field, case, 0, seed, root, points, values, proof) == (BAD, -7)
    assert _verify_raw(field, case, shift, seed, root, points, values, proof, raw_shift=_raw(p)) == (BAD, -7)
    flat_v = np.ascontiguousarray(orc.from_ints(field, [x for row in values for x in row]))
    flat_v[k * m - 1] = _raw(p)                                # an unreduced value, an unreduced point element
    assert _verify_raw(field, case, shift, seed, root, points, values, proof, raw_values=flat_v) == (BAD, -7)
    flat_z = np.ascontiguousarray(orc.from_ints(field, [x for z in points for x in z]))
    flat_z[n * m - 2] = _raw(p)
    assert _verify_raw(field, case, shift, seed, root, points, values, proof, raw_points=flat_z) == (BAD, -7)
    assert _verify_raw(field, case, shift, seed, root, points, values, proof, proof_len=len(proof) - 32) == (BAD, -7)
    two = zk_amd.two_adicity(field)
    big = (two, 1, 0, 1, 1, 1)   # n + b one past the two-adicity; the length is checked first, so the buffer has that length
    if two <= 40:
        buf = bytes(ref.proof_bytes(*big))
        assert _verify_raw(field, big, shift, seed, root, [[0] * two], [[0]], buf) == (NO_ROOT, -7)
    out = c.c_uint64(5)
    pb = _lib.lib.zk_mlbatch_proof_bytes
    for bad in ((0, 1, 1, 1, 0, 8), (4, 0, 1, 1, 1, 8), (4, 257, 1, 1, 1, 8), (4, 1, 0, 1, 1, 8), (4, 1, 17, 1, 1, 8), (4, 1, 1, 0, 1, 8),
                (4, 1, 1, 9, 1, 8), (4, 1, 1, 1, 4, 8), (4, 1, 1, 1, 1, 0), (4, 1, 1, 1, 1, 1025)):
        assert pb(*bad, c.byref(out)) == BAD and out.value == 5, bad
    assert pb(4, 1, 1, 1, 1, 8, None) == BAD
    assert pb(4, 256, 16, 1, 1, 8, c.byref(out)) == 0 and out.value == ref.proof_bytes(4, 1, 1, 8, 256, 16)
    assert _lib.lib.zk_mlbatch_free(None) == 0
