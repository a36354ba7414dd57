"""zk_zerocheck_prove / zk_zerocheck_verify_host / zk_mle_gate_sums / zk_bench_zerocheck on the device.  The reference has no zerocheck
argument: tests/zerocheck_ref.py is the definition.  In a child process every proof of the shared case list -- proof, point and claims
-- byte for byte against the definition on the three fields (n = 1 .. 13: one workgroup below m = 6, the first run kernel at m = 6, Lo
the whole weight up to m = 9, the first real Hi entries at m = 10 and 11, every shape with and without the fold), zk_mle_gate_sums of
every case against the definition and, for the gate x0, bit for bit against zk_mle_eq_sums.  In the parent one proof on the workload's
own scale (2^20: runs of 256 and 128 elements), repeated calls over stale pool blocks, the error table, the measurement hook, the C++
mirror and a gate check made of public calls only.  A wave takes a second run from n = 24 (k <= 8) or 23 on: out of a test's reach
(zerocheck_ref.SECOND_RUN_VARS); tools/zerocheck_bench.py runs that size."""
import os
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd._lib import c, lib, u8p, u64p, vpp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zerocheck_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from zerocheck_check import FIELD_IDS, X0_VARS, case_tail, digest  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "zerocheck_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BAD, MISMATCH = -20, -26
BIG_VARS, BIG_SEED = 20, 0x2C20


@pytest.fixture(scope="module")
def child():
    """{(kind, field id, key): (digest, verdict)}"""
    r = subprocess.run([sys.executable, CHECK], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert "zerocheck ok" in r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    return {(ln[0], ln[1], ln[2]): (ln[3], int(ln[4])) for ln in lines if ln and ln[0] in ("PROOF", "SUMS", "X0")}


@pytest.fixture(scope="module")
def expected():
    """the definition's digests and verdicts, computed once"""
    out = {}
    for case in ref.CASES:
        fi, gate, tables, seed = ref.case_inputs(case, worst_case_values)
        p = orc.modulus(fi)
        proof, point, claims = ref.prove(fi, gate, tables, seed)
        ok = ref.verify(fi, gate, case[0], seed, proof)
        assert (ok is not None) == (case[2] == 0) and (ok is None or ok == (point, claims)), case
        key = (FIELD_IDS[fi], ref.case_key(case))
        out[("PROOF",) + key] = (digest(proof + orc.from_ints(fi, point).tobytes() + orc.from_ints(fi, claims).tobytes()), int(ok is not None))
        out[("SUMS",) + key] = (digest(orc.from_ints(fi, ref.gate_sums(fi, gate, tables, case_tail(case, p))).tobytes()), 0)
    return out


def test_every_proof_against_the_definition(child, expected):
    """proof, point and claims of zk_zerocheck_prove against zerocheck_ref.prove, byte for byte, and zk_zerocheck_verify_host's verdict
    against zerocheck_ref.verify's (satisfying instances accepted with the prover's point and claims, the worst-case corpus rejected)"""
    want = {key: v for key, v in expected.items() if key[0] == "PROOF"}
    got = {key: v for key, v in child.items() if key[0] == "PROOF"}
    assert len(want) == len(ref.CASES) and set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, (wrong[:20], len(wrong))


def test_gate_sums_against_the_definition(child, expected):
    """the no-fold form at every m = 0 .. 12, and for the gate x0 bit for bit against the existing k_ml_round (asserted in the child)"""
    want = {key: v for key, v in expected.items() if key[0] == "SUMS"}
    got = {key: v for key, v in child.items() if key[0] == "SUMS"}
    assert set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, (wrong[:20], len(wrong))
    assert {key[1:] for key in child if key[0] == "X0"} == {(f, "n%d" % n) for f in FIELD_IDS for n in X0_VARS}


def _mul_tables(ctx, field, n):
    a, b = (orc.fill_random(field, BIG_SEED + i, 1 << n) for i in (0, 1))
    cc = orc.prod_reduce(field, n, [a, b])
    return [a, b, cc], [MLE.new(ctx, n, x) for x in (a, b, cc)]


def test_one_proof_on_the_workloads_scale():
    """BN254, n = 20, the gate x0 x1 - x2 on orc.fill_random's a, b and c = orc.prod_reduce(a, b): round 0 takes runs of 2^8 elements and
    round 1 of 2^7 (zerocheck_ref.RUN_GROWS_VARS = 19).  zk_zerocheck_verify_host accepts; the claims are the oracle's evaluations at the
    point; the tables are bit-identical afterwards"""
    field, n = FIELDS[0], BIG_VARS
    assert ref.RUN_GROWS_VARS <= n and ref.run_log(n - 1) == 8 and ref.run_log(n - 2) == 7 and min(ref.SECOND_RUN_VARS.values()) > 21
    ctx = zk_amd.Context(field, 0)
    g = zk_amd.Gate(field, 3, ref.GATES["mul"][1])
    srcs, tabs = _mul_tables(ctx, field, n)
    seed = bytes(range(32))
    proof, point, claims = zk_amd.zerocheck_prove(tabs, g, seed)
    got = zk_amd.zerocheck_verify(g, n, seed, proof)
    assert got is not None and np.array_equal(got[0], point) and np.array_equal(got[1], claims)
    for i, (s, t) in enumerate(zip(srcs, tabs)):
        assert np.array_equal(orc.mle_evaluate(field, n, s, point), claims[i]), i
        assert np.array_equal(t.evaluation_slice(), s), i
        t.free()
    ctx.close()


@pytest.fixture(params=range(3), ids=FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def test_repeated_calls_over_stale_pool_blocks(fctx):
    fi, field, ctx = fctx
    n, gate = 12, ref.GATES["plonk"]
    p = orc.modulus(field)
    import random
    tables = ref.satisfying_tables(gate, n, p, random.Random(77 + fi))
    srcs = [orc.from_ints(field, t) for t in tables]
    tabs = [MLE.new(ctx, n, s) for s in srcs]
    g = zk_amd.Gate(field, gate[0], gate[1])
    first = zk_amd.zerocheck_prove(tabs, g, bytes(32))
    for n_vars in list(range(0, 14)) * 2:
        MLE.random(ctx, n_vars, 31 + n_vars).free()
    again = zk_amd.zerocheck_prove(tabs, g, bytes(32))
    assert first[0] == again[0] and np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    assert all(np.array_equal(t.evaluation_slice(), s) for t, s in zip(tabs, srcs))
    assert zk_amd.zerocheck_verify(g, n, bytes(32), first[0]) is not None


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    n, gate = 6, ref.GATES["mul"]
    g, g_other = zk_amd.Gate(field, 3, gate[1]), zk_amd.Gate(zk_amd.BLS12_381_FR, 3, gate[1])
    tabs = [MLE.random(ctx, n, i) for i in range(3)]
    t_other, t0, t5 = MLE.random(other, n, 1), MLE.random(ctx, 0, 2), MLE.random(ctx, 5, 3)
    before = [t.evaluation_slice().copy() for t in tabs]

    def handles(ts):
        arr = (c.c_void_p * len(ts))(*[None if t is None else t._h for t in ts])
        return c.cast(arr, vpp), arr

    seed = np.arange(32, dtype=np.uint8)
    sp = seed.ctypes.data_as(u8p)
    buf = np.full(ref.proof_bytes(gate, n), 7, dtype=np.uint8)
    point, claims = np.full(4 * n, 9, dtype=np.uint64), np.full(4 * 3, 9, dtype=np.uint64)
    bp, zp, cp = buf.ctypes.data_as(u8p), point.ctypes.data_as(u64p), claims.ctypes.data_as(u64p)
    hp, _k0 = handles(tabs)
    pv = lib.zk_zerocheck_prove
    good = [ctx._h, hp, g._h, sp, bp, zp, cp]
    for i in range(7):   # every pointer
        bad = list(good)
        bad[i] = None
        assert pv(*bad) == BAD, i
    for ts, want in (([tabs[0], None, tabs[2]], BAD), ([tabs[0], t_other, tabs[2]], MISMATCH), ([tabs[0], tabs[1], t5], BAD),
                     ([t0, t0, t0], BAD)):
        hq, _k1 = handles(ts)
        assert pv(ctx._h, hq, g._h, sp, bp, zp, cp) == want, want
    hq, _k1 = handles([None, t_other, t5])
    assert pv(ctx._h, hq, g._h, sp, bp, zp, cp) == BAD            # a NULL table before another context
    hq, _k2 = handles([t_other, tabs[1], t5])
    assert pv(ctx._h, hq, g._h, sp, bp, zp, cp) == MISMATCH       # another context before the shapes
    assert pv(other._h, hp, g._h, sp, bp, zp, cp) == MISMATCH
    assert pv(ctx._h, hp, g_other._h, sp, bp, zp, cp) == BAD      # a gate of another field
    assert (buf == 7).all() and (point == 9).all() and (claims == 9).all()   # nothing was written by any of them
    assert pv(*good) == 0
    want = ref.prove(field, gate, [orc.to_ints(field, b) for b in before], seed.tobytes())
    assert (buf.tobytes(), orc.to_ints(field, point.reshape(n, 4)), orc.to_ints(field, claims.reshape(3, 4))) == want
    # zk_mle_gate_sums: a NULL tail with n > 1, a tail element that is not reduced
    sums = np.full(4 * 3, 9, dtype=np.uint64)
    tail = orc.from_ints(field, list(range(1, n)))
    raw_p = np.frombuffer(p.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    bad_tail = tail.copy()
    bad_tail[2] = raw_p
    gs = lib.zk_mle_gate_sums
    assert gs(ctx._h, hp, g._h, None, sums.ctypes.data_as(u64p)) == BAD and gs(ctx._h, hp, g._h, tail.ctypes.data_as(u64p), None) == BAD
    assert gs(ctx._h, hp, g._h, bad_tail.ctypes.data_as(u64p), sums.ctypes.data_as(u64p)) == BAD
    assert gs(other._h, hp, g._h, tail.ctypes.data_as(u64p), sums.ctypes.data_as(u64p)) == MISMATCH and (sums == 9).all()
    got = zk_amd.gate_sums(tabs, g, tail)
    assert orc.to_ints(field, got) == ref.gate_sums(field, gate, [orc.to_ints(field, b) for b in before], list(range(1, n)))
    # the measurement hook gives a time on its three paths and leaves the tables alone
    ms = c.c_double(-1.0)
    for path in (0, 1, 2):
        ms.value = -1.0
        assert lib.zk_bench_zerocheck(ctx._h, hp, g._h, path, 2, c.byref(ms)) == 0 and ms.value > 0, path
    assert zk_amd.bench_zerocheck(tabs, g, path=0, reps=1) > 0
    ms.value = -1.0
    bz = lib.zk_bench_zerocheck
    assert bz(ctx._h, hp, g._h, 3, 1, c.byref(ms)) == BAD and bz(ctx._h, hp, g._h, 0, 0, c.byref(ms)) == BAD
    assert bz(ctx._h, hp, g._h, 0, 1, None) == BAD and bz(ctx._h, None, g._h, 0, 1, c.byref(ms)) == BAD and bz(ctx._h, hp, None, 0, 1, c.byref(ms)) == BAD
    assert bz(other._h, hp, g._h, 0, 1, c.byref(ms)) == MISMATCH
    assert ms.value == -1.0 and all(np.array_equal(t.evaluation_slice(), b) for t, b in zip(tabs, before))
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_zerocheck.cpp over zk.hpp: gates, proofs, the verifier's verdicts, gate_sums, the errors"""
    exe = str(tmp_path / "test_zerocheck")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_zerocheck.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: zerocheck host tests passed" in r.stdout


def test_gate_check_from_public_calls():
    """eight Plonk columns at n = 6 under one batch commitment; seed = keccak of the root; the zerocheck; the k claims it leaves are
    opened from the commitment at the returned point and checked by mlbatch_verify.  With one witness entry changed the verdict is 0"""
    import random
    field, n, blowup, log_final, queries = zk_amd.BN254_FR, 6, 1, 0, 8
    p = orc.modulus(field)
    gate = ref.GATES["plonk"]
    ctx = zk_amd.Context(field, 0)
    g = zk_amd.Gate(field, gate[0], gate[1])
    one = orc.from_int(field, 1)
    columns = ref.satisfying_tables(gate, n, p, random.Random(6))

    def run(cols):
        tabs = [MLE.new(ctx, n, orc.from_ints(field, v)) for v in cols]
        com = zk_amd.MultilinearBatchCommitment.commit(tabs, blowup, one)
        root = com.root()
        seed = zk_amd.keccak256(root)   # binds all eight columns
        proof, _, _ = zk_amd.zerocheck_prove(tabs, g, seed)
        got = zk_amd.zerocheck_verify(g, n, seed, proof)   # the verifier: the argument, then the claims it leaves against the commitment
        if got is not None:
            values, opening = com.open(got[0][None], log_final, queries, seed)
            assert np.array_equal(np.asarray(values).reshape(gate[0], 4), got[1])
            assert zk_amd.mlbatch_verify(field, root, got[0][None], got[1][None], opening, blowup, log_final, queries, one, seed)
        for x in tabs + [com]:
            x.free()
        return got is not None

    assert run(columns)
    columns[2][17] = (columns[2][17] + 1) % p   # one entry of the witness column c
    assert not run(columns)
    ctx.close()
