"""zk_mlpcs_commit / zk_mlpcs_open / zk_mlpcs_verify_host / zk_mle_eq_sums / zk_bench_mlpcs_round on the device.  The reference has no
polynomial commitment: tests/mlpcs_ref.py is the definition.  In child processes under ZK_MLPCS_ROUND (the switch between the fused round
kernel and the eq-table route): every opening of the shared case list -- root, value and proof -- byte for byte against the definition, on
every setting; in the default child every zk_mle_eq_sums case (m = 0, both sides of a wave, no Hi table / one entry / two, both sides of a
workgroup; tail entries in {0, 1, p - 1, random}; worst-case limb patterns) against Python integers, and on BN254 the smallest table at
which the capped grid's loop takes a second trip (2^24 elements), and the run lengths below it, against the C oracle's arithmetic.  In
the parent three openings of one handle, the error table, the measurement hook and the C++ mirror."""
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
import mlpcs_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from mlpcs_check import BIG_SEED, SETTINGS, SWITCH, big_tail, case_key, digest  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "mlpcs_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
ARITY, NO_ROOT, BAD, MISMATCH = -2, -7, -20, -26


@pytest.fixture(scope="module")
def children():
    """{setting: {(kind, field id, key): digest}}: one child process per switch setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"mlpcs {setting} ok" in r.stdout
        lines = [ln.split() for ln in r.stdout.splitlines()]
        out[setting] = {(ln[0], ln[1], ln[2]): ln[3] for ln in lines if ln and ln[0] in ("SUMS", "BIGSUMS", "PROOF")}
    return out


@pytest.fixture(scope="module")
def expected_proofs():
    """{("PROOF", field id, key): digest of root + value + proof} from the definition, which also accepts each of them"""
    out = {}
    for case in ref.GPU_CASES:
        n, b, f, q = case
        fi = ref.case_field(case)
        table, shift, seed, z = ref.case_inputs(fi, case, worst_case_values)
        committed = ref.commit(fi, table, b, shift)
        root = ref.merkle_ref.root(committed[2])
        v, proof = ref.prove(fi, table, b, f, q, shift, seed, z, committed=committed)
        assert ref.verify(fi, n, b, f, q, shift, seed, root, z, v, proof), case   # the same bytes as the device's, below
        out[("PROOF", fri_ref.FIELD_IDS[fi], case_key(case))] = digest(root + orc.from_int(fi, v).tobytes() + proof)
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_opening_on_every_setting(children, expected_proofs, setting):
    """root, value (= t(z)) and proof of zk_mlpcs_commit / zk_mlpcs_open against mlpcs_ref.prove, byte for byte, with the fused round
    kernel, with the eq-table route and by default; zk_mlpcs_verify_host accepted each in the child, mlpcs_ref.verify in the fixture"""
    got = {key: dg for key, dg in children[setting].items() if key[0] == "PROOF"}
    assert len(expected_proofs) == len(ref.GPU_CASES) and set(got) == set(expected_proofs)
    wrong = sorted(key for key, want in expected_proofs.items() if got[key] != want)
    assert not wrong, (setting, wrong[:20], len(wrong))


def test_eq_sums_against_python_integers(children):
    """zk_mle_eq_sums on all three fields at every size of mlpcs_ref.EQ_SUMS_VARS; the other children run none (the call has no switch)"""
    got = {key: dg for key, dg in children["default"].items() if key[0] == "SUMS"}
    want = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for n in ref.EQ_SUMS_VARS:
            table, tail = ref.eq_sums_case(fi, n, worst_case_values)
            if n >= 8:
                assert {0, 1, p - 1} <= set(tail)
            want[("SUMS", fri_ref.FIELD_IDS[fi], "n%d" % n)] = digest(orc.from_ints(field, ref.eq_sums(table, tail, p)).tobytes())
    assert set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, wrong
    assert not any(key[0] != "PROOF" for setting in ("fused", "tables") for key in children[setting])


@pytest.mark.parametrize("n", ref.ORACLE_SUMS_VARS)
def test_eq_sums_against_the_oracle(children, n):
    """BN254 at the sizes Python integers are too slow for: runs of 2^7, 2^8 and 2^9 elements (n = 19, 20, 21) and n = 24, where 2^14 runs
    meet the capped grid's 2^13 waves and the loop takes a second trip.  The expected sums are the C oracle's: its generator's table (the
    one zk_mle_fill_random makes), each half evaluated at the tail"""
    field = FIELDS[0]
    assert ref.trips(ref.SECOND_TRIP_VARS) == 2 and ref.trips(ref.SECOND_TRIP_VARS - 1) == 1
    table = orc.fill_random(field, BIG_SEED + n, 1 << n)
    tail = orc.from_ints(field, big_tail(orc.modulus(field), n))
    half = 1 << (n - 1)
    want = np.stack([orc.mle_evaluate(field, n - 1, table[x * half:(x + 1) * half], tail) for x in range(2)])
    assert children["default"][("BIGSUMS", fri_ref.FIELD_IDS[0], "n%d" % n)] == digest(np.ascontiguousarray(want, dtype=np.uint64).tobytes())


@pytest.fixture(params=range(3), ids=fri_ref.FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def test_three_openings_of_one_handle(fctx):
    """the handle survives an open: openings at z1, z2 and z1 again give the definition's bytes, then another (f, Q); the root is
    unchanged; the source table may be freed after the commitment and is bit-identical after commit and after open when it is kept; the
    handle's blocks are cut from stale pool data, not zeros"""
    fi, field, ctx = fctx
    p = orc.modulus(field)
    case = (10, 2, 1, 8)
    n, b, f, q = case
    table, shift, seed, z1 = ref.case_inputs(fi, case, worst_case_values)
    sv, src = orc.from_int(field, shift), orc.from_ints(field, table)
    for n_vars in (9, 10, 11, 12, 13):
        MLE.random(ctx, n_vars, 77 + n_vars).free()
    kept, gone = MLE.new(ctx, n, src), MLE.new(ctx, n, src)
    com = zk_amd.MultilinearCommitment.commit(gone, b, sv)
    gone.free()
    com_kept = zk_amd.MultilinearCommitment.commit(kept, b, sv)
    assert np.array_equal(kept.evaluation_slice(), src)
    assert com.n_vars() == n
    committed = ref.commit(field, table, b, shift)
    root = com.root()
    assert root == ref.merkle_ref.root(committed[2]) == com_kept.root()
    z2 = [(7 * x + 3) % p for x in z1]
    for z in (z1, z2, z1):
        value, proof = com.open(orc.from_ints(field, z), f, q, seed)
        v, want = ref.prove(field, table, b, f, q, shift, seed, z, committed=committed)
        assert orc.to_int(field, value) == v and proof == want and len(proof) == zk_amd.mlpcs_proof_bytes(*case), z
        assert zk_amd.mlpcs_verify(field, root, orc.from_ints(field, z), value, proof, b, f, q, sv, seed)
        zb = [(z[0] + 1) % p] + list(z[1:])
        assert not zk_amd.mlpcs_verify(field, root, orc.from_ints(field, zb), value, proof, b, f, q, sv, seed)
    assert com.root() == root
    value, proof = com_kept.open(orc.from_ints(field, z2), 4, 3, seed)   # another final length and query count
    v, want = ref.prove(field, table, b, 4, 3, shift, seed, z2, committed=committed)
    assert orc.to_int(field, value) == v and proof == want
    assert np.array_equal(kept.evaluation_slice(), src) and com_kept.root() == root
    com.free()
    com_kept.free()


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    n = 6
    t, t_other, t0 = MLE.random(ctx, n, 1), MLE.random(other, n, 1), MLE.random(ctx, 0, 2)
    before = t.evaluation_slice().copy()
    five, zero = orc.from_int(field, 5), np.zeros(4, dtype=np.uint64)
    raw_p = np.frombuffer(p.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    fp, zp, pp = (x.ctypes.data_as(u64p) for x in (five, zero, raw_p))
    h = c.c_void_p()
    cm = lib.zk_mlpcs_commit
    # NULL, another context, the shapes, the shift, the domain -- in this order
    assert cm(ctx._h, None, 1, fp, c.byref(h)) == BAD and cm(ctx._h, t._h, 1, None, c.byref(h)) == BAD and cm(ctx._h, t._h, 1, fp, None) == BAD
    assert cm(ctx._h, t_other._h, 0, zp, c.byref(h)) == MISMATCH and cm(other._h, t._h, 1, fp, c.byref(h)) == MISMATCH
    for b in (0, 9):
        assert cm(ctx._h, t._h, b, fp, c.byref(h)) == BAD, b
    assert cm(ctx._h, t0._h, 1, fp, c.byref(h)) == BAD                             # n = 0
    assert cm(ctx._h, t._h, 1, zp, c.byref(h)) == BAD and cm(ctx._h, t._h, 1, pp, c.byref(h)) == BAD
    big = MLE.random(ctx, 21, 3)
    assert cm(ctx._h, big._h, 8, fp, c.byref(h)) == NO_ROOT                        # BN254: two-adicity 28
    big.free()
    assert not h.value
    com = zk_amd.MultilinearCommitment.commit(t, 1, five)
    seed = np.arange(32, dtype=np.uint8)
    sp = seed.ctypes.data_as(u8p)
    buf = np.full(ref.proof_bytes(n, 1, 0, 8), 7, dtype=np.uint8)
    val = np.full(4, 9, dtype=np.uint64)
    z = [0, 1, p - 1, 5, 6, 7]
    point = np.ascontiguousarray(orc.from_ints(field, z))
    bad_point = point.copy()
    bad_point[4] = raw_p
    bp, vp, zq, zbad = buf.ctypes.data_as(u8p), val.ctypes.data_as(u64p), point.ctypes.data_as(u64p), bad_point.ctypes.data_as(u64p)
    opn = lib.zk_mlpcs_open
    assert opn(ctx._h, com._h, None, n, 0, 8, sp, vp, bp) == BAD and opn(ctx._h, com._h, zq, n, 0, 8, None, vp, bp) == BAD
    assert opn(other._h, com._h, zq, n - 1, 0, 8, sp, vp, bp) == MISMATCH
    assert opn(ctx._h, com._h, zq, n - 1, 0, 8, sp, vp, bp) == ARITY and opn(ctx._h, com._h, zq, n + 1, 9, 8, sp, vp, bp) == ARITY
    for f, nq in ((n, 8), (n + 3, 8), (0, 0), (0, 1025)):
        assert opn(ctx._h, com._h, zq, n, f, nq, sp, vp, bp) == BAD, (f, nq)
    assert opn(ctx._h, com._h, zbad, n, 0, 8, sp, vp, bp) == BAD
    root_buf = np.zeros(32, dtype=np.uint8)
    assert lib.zk_mlpcs_root(other._h, com._h, root_buf.ctypes.data_as(u8p)) == MISMATCH
    sums = np.full(8, 9, dtype=np.uint64)
    sq = sums.ctypes.data_as(u64p)
    es = lib.zk_mle_eq_sums
    assert es(ctx._h, t._h, None, sq) == BAD and es(ctx._h, None, zq, sq) == BAD and es(ctx._h, t._h, zq, None) == BAD
    assert es(other._h, t._h, zq, sq) == MISMATCH and es(ctx._h, t0._h, zq, sq) == BAD
    assert es(ctx._h, t._h, zbad, sq) == BAD                                       # tail[4] is not reduced
    assert (buf == 7).all() and (val == 9).all() and (sums == 9).all() and not root_buf.any()   # nothing was written by any of them
    assert opn(ctx._h, com._h, zq, n, 0, 8, sp, vp, bp) == 0
    table = orc.to_ints(field, before)
    v, want = ref.prove(field, table, 1, 0, 8, 5, seed.tobytes(), z)
    assert buf.tobytes() == want and orc.to_int(field, val) == v
    assert es(ctx._h, t._h, zq, sq) == 0                                            # the first n - 1 elements of the point as a tail
    assert orc.to_ints(field, sums.reshape(2, 4)) == ref.eq_sums(table, z[:n - 1], p)
    one_var = MLE.new(ctx, 1, orc.from_ints(field, [3, p - 1]))
    assert orc.to_ints(field, zk_amd.eq_sums(one_var, [])) == [3, p - 1]             # m = 0: S_X = t[X], no tail
    # the measurement hook gives a time on every path and leaves the table alone
    ms = c.c_double(-1.0)
    for path in (0, 1, 2):
        ms.value = -1.0
        assert lib.zk_bench_mlpcs_round(ctx._h, t._h, path, 2, c.byref(ms)) == 0 and ms.value > 0, path
    assert zk_amd.bench_mlpcs_round(t, path=1, reps=1) > 0
    ms.value = -1.0
    assert lib.zk_bench_mlpcs_round(ctx._h, t._h, 3, 1, c.byref(ms)) == BAD and lib.zk_bench_mlpcs_round(ctx._h, t._h, 0, 0, c.byref(ms)) == BAD
    assert lib.zk_bench_mlpcs_round(other._h, t._h, 0, 1, c.byref(ms)) == MISMATCH and lib.zk_bench_mlpcs_round(ctx._h, t0._h, 0, 1, c.byref(ms)) == BAD
    assert ms.value == -1.0 and np.array_equal(t.evaluation_slice(), before)
    com.free()
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_mlpcs.cpp over zk.hpp: openings, the verifier's verdicts, several openings of one commitment, eq_sums, the errors"""
    exe = str(tmp_path / "test_mlpcs")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_mlpcs.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: mlpcs host tests passed" in r.stdout
