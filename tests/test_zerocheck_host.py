"""The definition of the zerocheck argument (tests/zerocheck_ref.py) checked on its own, and the host side of the library against it
without a GPU: zk_zerocheck_verify_host on the shared cases of the three fields (accepted proofs give the definition's point and claims;
one corrupted element per position class, a non-canonical element and a table with one violated row give a verdict of 0),
zk_gate_create's error table, zk_zerocheck_proof_bytes, the verifier at n = 40, the schedule constants, the new exports and their Python
signatures.  Everything is bytes."""
import ctypes as c
import os
import re
import resource
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zerocheck_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, BAD_FIELD = -20, -21
SYMBOLS = ("zk_gate_create", "zk_gate_free", "zk_gate_degree", "zk_gate_n_columns", "zk_zerocheck_proof_bytes", "zk_zerocheck_prove",
           "zk_zerocheck_verify_host", "zk_mle_gate_sums", "zk_bench_zerocheck")
WRAPPERS = ("Gate", "zerocheck_prove", "zerocheck_verify", "zerocheck_proof_bytes", "gate_sums", "bench_zerocheck")
UNTOUCHED = 0x0909090909090909
HOST_CASES = tuple(cs for cs in ref.CASES if cs[0] <= 8)
u32p = c.POINTER(c.c_uint32)


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _raw(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


def _gate(field, gate):
    return zk_amd.Gate(field, gate[0], gate[1])


def _verify_raw(g, n, seed, proof, proof_len=None):
    """(status, ok, point, claims): ints when accepted, else whether the buffers were left alone"""
    ok = c.c_int32(-7)
    point, claims = np.full((41, 4), UNTOUCHED, dtype=np.uint64), np.full((17, 4), UNTOUCHED, dtype=np.uint64)
    sd, pf = _u8(seed), _u8(proof)
    rc = _lib.lib.zk_zerocheck_verify_host(g._h, n, sd.ctypes.data_as(_lib.u8p), pf.ctypes.data_as(_lib.u8p), len(proof) if proof_len is None else proof_len,
                                           point.ctypes.data_as(_lib.u64p), claims.ctypes.data_as(_lib.u64p), c.byref(ok))
    if rc == 0 and ok.value == 1:
        assert (point[n:] == UNTOUCHED).all() and (claims[g.k:] == UNTOUCHED).all()
        return rc, 1, orc.to_ints(g.field, point[:n]), orc.to_ints(g.field, claims[:g.k])
    return rc, ok.value, bool((point == UNTOUCHED).all()), bool((claims == UNTOUCHED).all())


def _both(g, gate, n, seed, proof):
    rc, ok, point, claims = _verify_raw(g, n, seed, proof)
    want = ref.verify(g.field, gate, n, seed, proof)
    assert rc == 0 and ok == int(want is not None), (n, rc, ok, want)
    if want is None:
        assert point is True and claims is True   # nothing was written
        return None
    assert (point, claims) == (list(want[0]), list(want[1]))
    return want


def _put(proof, at, value):
    return proof[:at] + int(value).to_bytes(32, "big") + proof[at + 32:]


@pytest.fixture(scope="module")
def proofs():
    """{case: (field, gate, tables, seed, proof, point, claims)} from the definition, computed once"""
    out = {}
    for case in HOST_CASES:
        field, gate, tables, seed = ref.case_inputs(case, worst_case_values)
        out[case] = (field, gate, tables, seed) + ref.prove(field, gate, tables, seed)
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
    assert re.search(r"^OBJS := .*\bzerocheck\.o\b", make, flags=re.M)


def test_case_lists_and_schedule_constants():
    assert {cs[0] for cs in ref.CASES} == set(range(1, 14)) and {cs[1] for cs in ref.CASES} == set(ref.GATE_NAMES)
    assert {ref.case_field(cs) for cs in ref.CASES} == {0, 1, 2} and {cs[2] for cs in ref.CASES} == {0, 1}
    assert {ref.case_field(cs) for cs in HOST_CASES} == {0, 1, 2} and {cs[1] for cs in HOST_CASES} == set(ref.GATE_NAMES)
    assert {name: (g[0], len(g[1]), ref.gate_degree(g)) for name, g in ref.GATES.items()} == {
        "x0": (1, 1, 1), "mul": (3, 2, 2), "plonk": (8, 5, 3), "deg6": (3, 2, 6), "limits": (16, 32, 6), "const": (4, 4, 2)}
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "zerocheck_kernels.cuh")).read()
    ml = open(os.path.join(ROOT, "zk_amd", "csrc", "mlpcs_kernels.cuh")).read()
    core = open(os.path.join(ROOT, "zk_amd", "csrc", "host_core.hpp")).read()
    limits = re.search(r"kZcMaxCols = (\d+), kZcMaxTerms = (\d+), kZcMaxDegree = (\d+), kZcMaxMentions = (\d+);", src).groups()
    assert tuple(int(x) for x in limits) == (ref.MAX_COLS, ref.MAX_TERMS, ref.MAX_DEGREE, ref.MAX_MENTIONS)
    assert ref.WIDE_COLS == int(re.search(r"kZcWideCols = (\d+);", src).group(1))
    assert ref.LO_BITS == int(re.search(r"constexpr uint32_t kMlLoBits = (\d+);", ml).group(1))
    assert ref.RUN_MIN_BITS == int(re.search(r"constexpr uint32_t kMlRunMinBits = (\d+);", ml).group(1))
    assert ref.RUNS_TARGET_LOG == int(re.search(r"constexpr uint32_t kMlRunsTargetLog = (\d+);", ml).group(1))
    assert ref.MAX_BLOCKS == int(re.search(r"constexpr uint32_t kMaxGrid = (\d+);", core).group(1))
    assert ref.MAX_VARS == int(re.search(r"constexpr uint64_t kMaxVars = (\d+);", core).group(1))
    # the shapes a proof of n = 13 passes: one workgroup below m = 6, the first run kernel at 6, Lo the whole weight up to 9, Hi from 10
    assert [ref.run_log(m) for m in range(13)] == [None] * 6 + [6] * 7
    assert ref.RUN_GROWS_VARS == 19 and ref.run_log(18) == 7 and ref.run_log(19) == 8
    assert ref.SECOND_RUN_VARS == {8: 24, 16: 23}


def test_completeness_and_proof_bytes(proofs):
    for case, (field, gate, tables, seed, proof, point, claims) in proofs.items():
        n, p = case[0], orc.modulus(field)
        g = _gate(field, gate)
        assert g.degree() == ref.gate_degree(gate) and g.n_columns() == gate[0]
        assert len(proof) == ref.proof_bytes(gate, n) == zk_amd.zerocheck_proof_bytes(g, n) == 32 * (n * (g.degree() + 1) + g.k), case
        assert [ref.evaluate(t, point, p) for t in tables] == claims, case   # the claims that are left are true
        got = _both(g, gate, n, seed, proof)
        if case[2] == 0:   # a satisfying instance: accepted, with the definition's point and claims
            assert got == (point, claims), case
            out = zk_amd.zerocheck_verify(g, n, seed, proof)
            assert out is not None and orc.to_ints(field, out[0]) == point and orc.to_ints(field, out[1]) == claims
        else:              # the worst-case corpus does not satisfy the gate
            assert got is None and zk_amd.zerocheck_verify(g, n, seed, proof) is None, case
    assert {cs[2] for cs in proofs} == {0, 1}


def test_every_change_is_rejected_by_both(proofs):
    for case, (field, gate, tables, seed, proof, point, claims) in proofs.items():
        if case[2]:
            continue
        n, p = case[0], orc.modulus(field)
        g = _gate(field, gate)
        for name, at in ref.section_offsets(gate, n).items():   # one element per position class: a g_j(0), a g_j(d), a final value
            bad = bytearray(proof)
            bad[at + 31] ^= 1
            assert _both(g, gate, n, seed, bytes(bad)) is None, (case, name)
            assert _both(g, gate, n, seed, _put(proof, at, p)) is None, (case, name)            # an element >= p
            assert _both(g, gate, n, seed, _put(proof, at, (1 << 256) - 1)) is None, (case, name)
        if n >= 2 and any(proof):   # another seed is another tau (the gate x0's satisfying table is zero, and so is its proof, under any seed)
            assert _both(g, gate, n, bytes([seed[0] ^ 1]) + seed[1:], proof) is None, case
        for other in (proof[:-1], proof + b"\0", proof[:-32], proof + proof[-32:]):
            assert ref.verify(field, gate, n, seed, other) is None
            assert _verify_raw(g, n, seed, other) == (BAD, -7, True, True)
        # one violated row: the prover makes the definition's bytes, and both verifiers reject them
        broken = [list(t) for t in tables]
        row, col = (3 * n) % (1 << n), next(f for cf, cols in ref.gate_mod(gate, p)[1] if cf for f in cols)
        broken[col][row] = (broken[col][row] + 1) % p
        if ref.gate_eval(ref.gate_mod(gate, p)[1], [t[row] for t in broken], p):
            assert _both(g, gate, n, seed, ref.prove(field, gate, broken, seed)[0]) is None, case


def test_gate_create_error_table():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    one = orc.from_int(field, 1)

    def create(fld, k, terms, raw_coeffs=None, null=()):
        coeffs = raw_coeffs if raw_coeffs is not None else np.ascontiguousarray(np.stack([orc.from_int(field, cf) for cf, _ in terms] or [one]))
        lens = np.array([len(cols) for _, cols in terms] or [0], dtype=np.uint32)
        flat = np.array([f for _, cols in terms for f in cols] or [0], dtype=np.uint32)
        h = c.c_void_p()
        args = [fld, k, len(terms), coeffs.ctypes.data_as(_lib.u64p), lens.ctypes.data_as(u32p), flat.ctypes.data_as(u32p), c.byref(h)]
        for i in null:
            args[i] = None
        rc = _lib.lib.zk_gate_create(*args)
        if rc == 0:
            _lib.lib.zk_gate_free(h)
        else:
            assert not h.value   # nothing was written
        return rc

    good = [(1, (0, 1)), (p - 1, (2,))]
    assert create(field, 3, good) == 0
    for i in (3, 4, 5, 6):
        assert create(field, 3, good, null=(i,)) == BAD, i
    assert create(7, 3, good, null=(3,)) == BAD and create(7, 0, good) == BAD_FIELD   # a NULL first, the field before the shapes
    assert create(field, 0, good) == BAD and create(field, 17, good) == BAD and create(field, 16, good) == 0
    assert create(field, 3, []) == BAD and create(field, 1, [(1, (0,))] * 33) == BAD and create(field, 1, [(1, (0,))] * 32) == 0
    assert create(field, 1, [(1, (0,) * 7)]) == BAD and create(field, 1, [(1, (0,) * 6)]) == 0                 # a term's length
    assert create(field, 2, [(1, (0, 1, 0))] * 22) == BAD and create(field, 2, [(1, (0, 1))] * 32) == 0         # 66 and 64 mentions
    assert create(field, 3, [(1, (0, 3))]) == BAD                                                               # a factor >= k
    assert create(field, 3, [(5, ())]) == BAD and create(field, 3, [(5, ()), (1, ())]) == BAD                   # d = 0
    bad_coeffs = np.ascontiguousarray(np.stack([one, _raw(p)]))
    assert create(field, 3, good, raw_coeffs=bad_coeffs) == BAD                                                 # a coefficient >= p
    d = c.c_uint32(9)
    assert _lib.lib.zk_gate_degree(None, c.byref(d)) == BAD and _lib.lib.zk_gate_n_columns(None, c.byref(d)) == BAD and d.value == 9
    g = zk_amd.Gate(field, 3, good)
    assert _lib.lib.zk_gate_degree(g._h, None) == BAD and _lib.lib.zk_gate_n_columns(g._h, None) == BAD
    assert _lib.lib.zk_gate_free(None) == 0
    with pytest.raises(zk_amd.ZkError):
        zk_amd.Gate(field, 3, [(1, (0, 3))])


def test_verifier_argument_table_and_proof_bytes(proofs):
    case = next(cs for cs in HOST_CASES if cs[2] == 0 and cs[0] >= 3)
    field, gate, tables, seed, proof, point, claims = proofs[case]
    n = case[0]
    g = _gate(field, gate)
    assert _verify_raw(g, n, seed, proof)[:2] == (0, 1)
    sd, pf = _u8(seed), _u8(proof)
    pt, cl, ok = np.full((n, 4), UNTOUCHED, dtype=np.uint64), np.full((g.k, 4), UNTOUCHED, dtype=np.uint64), c.c_int32(-7)
    args = [g._h, n, sd.ctypes.data_as(_lib.u8p), pf.ctypes.data_as(_lib.u8p), len(proof), pt.ctypes.data_as(_lib.u64p), cl.ctypes.data_as(_lib.u64p),
            c.byref(ok)]
    for i in (0, 2, 3, 5, 6, 7):
        bad = list(args)
        bad[i] = None
        assert _lib.lib.zk_zerocheck_verify_host(*bad) == BAD, i
    assert (pt == UNTOUCHED).all() and (cl == UNTOUCHED).all() and ok.value == -7
    for bad_n in (0, 41):
        assert _verify_raw(g, bad_n, seed, proof) == (BAD, -7, True, True)
    assert _verify_raw(g, n, seed, proof, proof_len=len(proof) - 32) == (BAD, -7, True, True)
    for m in (n - 1, n + 1):
        assert _verify_raw(g, m, seed, proof) == (BAD, -7, True, True)
    out = c.c_uint64(5)
    for bad_n in (0, 41, 1 << 31):
        assert _lib.lib.zk_zerocheck_proof_bytes(g._h, bad_n, c.byref(out)) == BAD and out.value == 5
    assert _lib.lib.zk_zerocheck_proof_bytes(g._h, 4, None) == BAD and _lib.lib.zk_zerocheck_proof_bytes(None, 4, c.byref(out)) == BAD
    assert _lib.lib.zk_zerocheck_proof_bytes(g._h, 40, c.byref(out)) == 0 and out.value == 32 * (40 * (g.degree() + 1) + g.k)


def test_verifier_at_forty_variables_allocates_nothing_sized_by_n():
    """n = 40: the verifier runs (a table of 2^40 elements would be 32 TiB), gives the definition's verdict on a proof of zeros -- which
    the gate x0 accepts: every g_j = 0, every claim 0 -- and rejects it with one element changed; the process's peak memory does not move"""
    field, gate = zk_amd.BLS12_381_FR, ref.GATES["x0"]
    g = _gate(field, gate)
    n = 40
    proof = bytes(ref.proof_bytes(gate, n))
    seed = bytes(range(32))
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    want = ref.verify(field, gate, n, seed, proof)
    assert want is not None and want[1] == [0] and len(want[0]) == n
    assert _both(g, gate, n, seed, proof) == want
    assert _both(g, gate, n, seed, _put(proof, 32 * 5, 1)) is None
    plonk = ref.GATES["plonk"]
    assert _both(_gate(field, plonk), plonk, n, seed, bytes(ref.proof_bytes(plonk, n))) is not None
    assert resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before < 64 * 1024   # KiB
