"""zk_perm_prove / zk_perm_verify_host / zk_mle_perm_fingerprint / zk_bench_perm on the device.  The reference has no permutation
argument: tests/perm_ref.py is the definition.  In a child process every proof of the shared case list -- proof, point and claims --
byte for byte against the definition on the three fields: N <= 10 (the LDS stage alone), N = 11 .. 14 (one, two, three and four levels
above it), kappa = 0 .. 4, padding columns (k = 3, 5, 9), one instance with a broken copy; the fingerprint table bit for bit; the head
of the proof against zk_gprod_prove on that table.  More children force the fused route (ZK_PERM_FUSE=1: at N = 11 .. 14 one launch of
k_perm_tree<1>, <2>, <2> and a k_ptree<1>, <2> and a k_ptree<2>; fused levels that are column bits at k = 5, 8, 9, 16, that straddle
column and row bits at k = 2 and that are row bits at k = 1) under every ZK_GPROD_TREE_FUSE and under a grid of one workgroup
(ZK_PERM_MAX_GRID=1: four trips of the wave loop at N = 13), ZK_PERM_FUSE=0 and the unfused route one level per launch, and must give
the default route's digests.  In the parent repeated calls over stale pool blocks, the error table, the measurement hook, the C++ mirror and a Plonk
circuit proven end to end from public calls only."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd._lib import c, lib, u8p, u64p, vpp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perm_ref as ref  # noqa: E402
import zerocheck_ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from perm_check import FIELD_IDS, digest  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "perm_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BAD, MISMATCH = -20, -26
SWITCHES = ("ZK_PERM_FUSE", "ZK_GPROD_TREE_FUSE", "ZK_PERM_MAX_GRID")
FUSED = {"ZK_PERM_FUSE": "1"}
ROUTES = (FUSED, dict(FUSED, ZK_GPROD_TREE_FUSE="1"), dict(FUSED, ZK_GPROD_TREE_FUSE="2"), dict(FUSED, ZK_GPROD_TREE_FUSE="3"),
          dict(FUSED, ZK_PERM_MAX_GRID="1"), {"ZK_PERM_FUSE": "0"}, {"ZK_GPROD_TREE_FUSE": "1"})


def _run_child(which, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    r = subprocess.run([sys.executable, CHECK, which], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert "perm ok" in r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    return {(ln[0], ln[1], ln[2]): (ln[3], int(ln[4])) for ln in lines if ln and ln[0] in ("PROOF", "FP", "HEAD")}


@pytest.fixture(scope="module")
def child():
    """{(kind, field id, key): (digest, verdict)} on the default route"""
    return _run_child("all", {})


@pytest.fixture(scope="module")
def expected():
    """the definition's digests and verdicts, computed once"""
    out = {}
    for case in ref.GPU_CASES:
        fi, w, sigma, beta, gamma, seed = ref.case_inputs(case, worst_case_values)
        proof, point, claims = ref.prove(fi, w, sigma, beta, gamma, seed)
        ok = ref.verify(fi, case[0], case[1], beta, gamma, seed, proof)
        assert (ok is not None) == (case[3] == 0) and (ok is None or ok == (point, claims)), case
        key = (FIELD_IDS[fi], ref.case_key(case))
        out[("PROOF",) + key] = (digest(proof + orc.from_ints(fi, point).tobytes() + orc.from_ints(fi, claims).tobytes()), int(ok is not None))
        out[("FP",) + key] = (digest(orc.from_ints(fi, ref.fingerprint(fi, w, sigma, beta, gamma)).tobytes()), 0)
    return out


def test_case_list_covers_the_kernel_shapes():
    import gprod_ref
    total = {ref.total_vars(cs[0], cs[1]) for cs in ref.GPU_CASES}
    assert {11, 12, 13, 14} <= total and min(total) <= 4 and {ref.kappa(cs[1]) for cs in ref.GPU_CASES} == {0, 1, 2, 3, 4}
    assert all(ref.total_vars(cs[0], cs[1]) <= gprod_ref.LDS_VARS for cs in ref.GPU_SMALL_CASES)
    assert all(ref.total_vars(cs[0], cs[1]) > gprod_ref.LDS_VARS and cs[0] >= 6 for cs in ref.GPU_FUSED_CASES)
    assert {1, 2, 3, 5, 8, 9, 16} <= {cs[1] for cs in ref.GPU_CASES} and {cs[3] for cs in ref.GPU_CASES} == {0, 1}
    assert {ref.case_field(cs) for cs in ref.GPU_CASES} == {0, 1, 2}
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "perm_kernels.cuh")).read()
    assert "constexpr uint32_t kPermMaxCols = %d;" % ref.MAX_COLS in src and "constexpr uint32_t kPermMaxFuse = 2;" in src


def test_every_proof_against_the_definition(child, expected):
    """proof, point and claims of zk_perm_prove against perm_ref.prove, byte for byte, and zk_perm_verify_host's verdict against
    perm_ref.verify's (satisfied wiring accepted with the prover's point and claims, the broken copy rejected with the bytes still equal)"""
    want = {key: v for key, v in expected.items() if key[0] == "PROOF"}
    got = {key: v for key, v in child.items() if key[0] == "PROOF"}
    assert len(want) == len(ref.GPU_CASES) and set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, (wrong[:20], len(wrong))
    assert sorted(v[1] for v in want.values()).count(0) == 1


def test_fingerprint_against_the_definition(child, expected):
    want = {key: v for key, v in expected.items() if key[0] == "FP"}
    got = {key: v for key, v in child.items() if key[0] == "FP"}
    assert set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, (wrong[:20], len(wrong))


def test_head_is_the_grand_product_of_the_fingerprint(child):
    """zk_gprod_prove on zk_mle_perm_fingerprint's table under seed' gives the head of zk_perm_prove's proof and its point (asserted in
    the child, for every case: no reference involved)"""
    assert {key[1:] for key in child if key[0] == "HEAD"} == {(FIELD_IDS[ref.case_field(cs)], ref.case_key(cs)) for cs in ref.GPU_CASES}


@pytest.mark.parametrize("env", ROUTES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_every_route_makes_the_same_bytes(child, env):
    """ZK_PERM_FUSE=1 alone and with ZK_GPROD_TREE_FUSE=1, 2, 3 (k_perm_tree<1>, <2>, <2> and the tree's own launches behind it) and with
    ZK_PERM_MAX_GRID=1 (every wave of one workgroup loops over its runs); ZK_PERM_FUSE=0 (k_perm_leaves, then the tree over F: the
    default, spelled out); the default route with the tree one level per launch"""
    got = _run_child("fused", env)
    assert len(got) == 3 * len(ref.GPU_FUSED_CASES)
    wrong = sorted(key for key in got if got[key] != child[key])
    assert not wrong, (env, wrong[:20])


@pytest.fixture(params=range(3), ids=FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def _columns(ctx, field, n, k, seed):
    """(ints w, ints sigma, source arrays, tables): satisfied wiring from random classes"""
    p = orc.modulus(field)
    rng = random.Random(seed)
    classes = np.array([[rng.randrange(max(1, k << (n - 1))) for _ in range(1 << n)] for _ in range(k)])
    value = {}
    w = [[value.setdefault(int(cid), rng.randrange(p)) for cid in col] for col in classes]
    sigma = zk_amd.wiring_sigma(classes).tolist()
    srcs = [orc.from_ints(field, t) for t in w + sigma]
    return w, sigma, srcs, [MLE.new(ctx, n, s) for s in srcs]


def test_repeated_calls_over_stale_pool_blocks(fctx):
    fi, field, ctx = fctx
    n, k = 9, 3
    w, sigma, srcs, tabs = _columns(ctx, field, n, k, 50 + fi)
    beta, gamma = orc.from_int(field, 1234567 + fi), orc.from_int(field, 7654321)
    first = zk_amd.permutation_prove(tabs[:k], tabs[k:], beta, gamma, bytes(32))
    for n_vars in list(range(0, 14)) * 2:
        MLE.random(ctx, n_vars, 31 + n_vars).free()
    again = zk_amd.permutation_prove(tabs[:k], tabs[k:], beta, gamma, bytes(32))
    assert first[0] == again[0] and np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    assert all(np.array_equal(t.evaluation_slice(), s) for t, s in zip(tabs, srcs))   # the inputs are left intact
    got = zk_amd.permutation_verify(field, n, k, beta, gamma, bytes(32), first[0])
    assert got is not None and np.array_equal(got[0], first[1]) and np.array_equal(got[1], first[2])
    for i, t in enumerate(tabs):
        assert np.array_equal(t.evaluate(first[1]), first[2][i]), i


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    n, k = 5, 2
    w, sigma, srcs, tabs = _columns(ctx, field, n, k, 9)
    t_other, t0, t4 = MLE.random(other, n, 1), MLE.random(ctx, 0, 2), MLE.random(ctx, 4, 3)

    def handles(ts):
        arr = (c.c_void_p * len(ts))(*[None if t is None else t._h for t in ts])
        return c.cast(arr, vpp), arr

    seed = np.arange(32, dtype=np.uint8)
    sp = seed.ctypes.data_as(u8p)
    beta, gamma = orc.from_int(field, 11), orc.from_int(field, 13)
    raw_p = np.frombuffer(p.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    bp_, gp_, rp_ = (x.ctypes.data_as(u64p) for x in (beta, gamma, raw_p))
    buf = np.full(ref.proof_bytes(n, k), 7, dtype=np.uint8)
    point, claims = np.full(4 * n, 9, dtype=np.uint64), np.full(4 * 2 * k, 9, dtype=np.uint64)
    bp, zp, cp = buf.ctypes.data_as(u8p), point.ctypes.data_as(u64p), claims.ctypes.data_as(u64p)
    wp, _k0 = handles(tabs[:k])
    sg, _k1 = handles(tabs[k:])
    pv = lib.zk_perm_prove
    good = [ctx._h, wp, sg, k, bp_, gp_, sp, bp, zp, cp]
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9):   # every pointer
        bad = list(good)
        bad[i] = None
        assert pv(*bad) == BAD, i

    def with_w(ts, kk=k, sig=None):
        hq, _keep = handles(ts)
        hs, _keep2 = handles(sig) if sig is not None else (sg, None)
        return pv(ctx._h, hq, hs, kk, bp_, gp_, sp, bp, zp, cp)

    assert with_w([tabs[0], None]) == BAD and with_w([tabs[0], t_other]) == MISMATCH and with_w([tabs[0], t4]) == BAD
    assert with_w([None, t_other]) == BAD                     # a NULL table before another context
    assert with_w([t_other, t4]) == MISMATCH                  # another context before the shapes
    assert with_w(tabs[:k], sig=[tabs[2], None]) == BAD and with_w(tabs[:k], sig=[tabs[2], t_other]) == MISMATCH
    assert with_w(tabs[:k], sig=[tabs[2], t4]) == BAD
    assert with_w([t0, t0], sig=[t0, t0]) == BAD              # n_vars = 0
    assert with_w(tabs[:k], kk=0) == BAD and with_w([tabs[0]] * 17, kk=17, sig=[tabs[2]] * 17) == BAD
    assert pv(other._h, wp, sg, k, bp_, gp_, sp, bp, zp, cp) == MISMATCH
    assert pv(ctx._h, wp, sg, k, rp_, gp_, sp, bp, zp, cp) == BAD and pv(ctx._h, wp, sg, k, bp_, rp_, sp, bp, zp, cp) == BAD
    assert (buf == 7).all() and (point == 9).all() and (claims == 9).all()   # nothing was written by any of them
    assert pv(*good) == 0
    want = ref.prove(field, w, sigma, 11, 13, seed.tobytes())
    assert (buf.tobytes(), orc.to_ints(field, point.reshape(n, 4)), orc.to_ints(field, claims.reshape(2 * k, 4))) == want
    # zk_mle_perm_fingerprint
    h = c.c_void_p()
    fp = lib.zk_mle_perm_fingerprint
    assert fp(ctx._h, wp, sg, k, bp_, gp_, None) == BAD and fp(ctx._h, None, sg, k, bp_, gp_, c.byref(h)) == BAD
    assert fp(ctx._h, wp, sg, k, rp_, gp_, c.byref(h)) == BAD and fp(other._h, wp, sg, k, bp_, gp_, c.byref(h)) == MISMATCH and not h.value
    # (N > 40 needs columns of 2^36 elements: tests/test_perm_host.py covers that limit on the verifier and on zk_perm_proof_bytes)
    # the measurement hook gives a time on its four paths and leaves the columns alone
    ms = c.c_double(-1.0)
    for path in (0, 1, 2, 3):
        ms.value = -1.0
        assert lib.zk_bench_perm(ctx._h, wp, sg, k, path, 2, c.byref(ms)) == 0 and ms.value > 0, path
    assert zk_amd.bench_perm(tabs[:k], tabs[k:], path=0, reps=1) > 0
    w12, s12, _, tabs12 = _columns(ctx, field, 11, 2, 10)   # a shape with a fused launch
    assert all(zk_amd.bench_perm(tabs12[:2], tabs12[2:], path=path, reps=1) > 0 for path in (0, 1, 2, 3))
    ms.value = -1.0
    bz = lib.zk_bench_perm
    assert bz(ctx._h, wp, sg, k, 4, 1, c.byref(ms)) == BAD and bz(ctx._h, wp, sg, k, 0, 0, c.byref(ms)) == BAD
    assert bz(ctx._h, wp, sg, k, 0, 1, None) == BAD and bz(ctx._h, None, sg, k, 0, 1, c.byref(ms)) == BAD and bz(ctx._h, wp, None, k, 0, 1, c.byref(ms)) == BAD
    assert bz(other._h, wp, sg, k, 0, 1, c.byref(ms)) == MISMATCH
    assert ms.value == -1.0 and all(np.array_equal(t.evaluation_slice(), s) for t, s in zip(tabs, srcs))
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_perm.cpp over zk.hpp: proofs, the verifier's verdicts, the fingerprint table, the errors"""
    exe = str(tmp_path / "test_perm")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_perm.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: permutation host tests passed" in r.stdout


def _plonk_circuit(n, p, rng):
    """a vanilla Plonk circuit of 2^n rows over variables: each row multiplies or adds two earlier variables into a new one.  Returns the
    eight gate columns (a, b, c, qL, qR, qM, qO, qC) and the (3, 2^n) copy classes of a, b, c: the variable each cell holds"""
    values = [rng.randrange(p) for _ in range(4)]
    cols = [[] for _ in range(8)]
    classes = [[], [], []]
    for _ in range(1 << n):
        ia, ib = rng.randrange(len(values)), rng.randrange(len(values))
        mul = rng.random() < 0.5
        values.append(values[ia] * values[ib] % p if mul else (values[ia] + values[ib]) % p)
        row = (values[ia], values[ib], values[-1], 0 if mul else 1, 0 if mul else 1, 1 if mul else 0, p - 1, 0)
        for col, x in zip(cols, row):
            col.append(x)
        for cl, var in zip(classes, (ia, ib, len(values) - 1)):
            cl.append(var)
    return cols, np.array(classes)


def test_plonk_gates_and_wiring_from_public_calls():
    """n = 6 on BN254: witness, selectors and sigma under ONE batch commitment; the seed from its root, beta and gamma from a transcript
    over the seed; the zerocheck and the permutation argument; ONE batch opening at their two points, against which both verifiers'
    claims are checked.  With one copy broken (the gate still holds on every row) the permutation verifier rejects"""
    field, n, blowup, log_final, queries = zk_amd.BN254_FR, 6, 1, 0, 8
    p = orc.modulus(field)
    gate = zerocheck_ref.GATES["plonk"]
    ctx = zk_amd.Context(field, 0)
    g = zk_amd.Gate(field, gate[0], gate[1])
    one = orc.from_int(field, 1)
    cols, classes = _plonk_circuit(n, p, random.Random(66))
    sigma = zk_amd.wiring_sigma(classes)
    assert sorted(sigma.reshape(-1).tolist()) == list(range(3 << n)) and (sigma != np.arange(3 << n).reshape(3, -1)).any()

    def run(gate_cols):
        tabs = [MLE.new(ctx, n, orc.from_ints(field, v)) for v in gate_cols] + [MLE.new(ctx, n, orc.from_ints(field, row)) for row in sigma.tolist()]
        com = zk_amd.MultilinearBatchCommitment.commit(tabs, blowup, one)   # columns 0..2 witness, 3..7 selectors, 8..10 sigma
        root = com.root()
        seed = zk_amd.keccak256(root)
        tr = zk_amd.Transcript()
        tr.append(seed)
        beta, gamma = tr.sample_field_element(field), tr.sample_field_element(field)
        zc_proof, _, _ = zk_amd.zerocheck_prove(tabs[:8], g, seed)
        pm_proof, _, _ = zk_amd.permutation_prove(tabs[:3], tabs[8:], beta, gamma, seed)
        zc = zk_amd.zerocheck_verify(g, n, seed, zc_proof)
        pm = zk_amd.permutation_verify(field, n, 3, beta, gamma, seed, pm_proof)
        if zc is not None and pm is not None:
            points = np.stack([zc[0], pm[0]])
            values, opening = com.open(points, log_final, queries, seed)   # ONE opening at the two points
            values = np.asarray(values).reshape(2, 11, 4)
            assert np.array_equal(values[0][:8], zc[1])
            assert np.array_equal(values[1][:3], pm[1][:3]) and np.array_equal(values[1][8:], pm[1][3:])
            assert zk_amd.mlbatch_verify(field, root, points, values, opening, blowup, log_final, queries, one, seed)
        for x in tabs + [com]:
            x.free()
        return zc is not None, pm is not None

    assert run(cols) == (True, True)
    # row r reads a variable as its a; feed it another value and repair the row's output: every gate holds, one copy does not
    r = next(i for i in range(1 << n) if cols[5][i] == 0)   # an addition row
    broken = [list(col) for col in cols]
    broken[0][r] = (broken[0][r] + 1) % p
    broken[2][r] = (broken[2][r] + 1) % p
    assert run(broken) == (True, False)
    ctx.close()
