"""zk_mle_product_tree / zk_gprod_prove / zk_gprod_verify_host / zk_bench_gprod on the device.  The reference has no grand-product
argument: tests/gprod_ref.py is the definition.  In child processes under ZK_GPROD_TREE_FUSE (the levels of the product tree per launch):
every proof of the shared case list -- product, proof, point and claim -- byte for byte against the definition, on every setting; every
tree from 2 elements to two levels past the LDS stage on the three fields with a NULL shift and with p - 1 against Python integers; on
BN254 the tree over 2^20 elements, and with one level per launch over the smallest table at which the capped grid takes a second trip
(2^24), against the C oracle's arithmetic.  In the parent one proof on the workload's own scale (2^20), repeated calls over stale pool
blocks, the error table, the measurement hook, the C++ mirror and a permutation check made of public calls only."""
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
import gprod_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from gprod_check import BIG_SEED, BIG_VARS, FIELD_IDS, SETTINGS, SWITCH, big_vars, case_key, digest, oracle_heap, tree_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "gprod_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BAD, MISMATCH = -20, -26


@pytest.fixture(scope="module")
def children():
    """{setting: {(kind, field id, key): digest}}: one child process per switch setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"gprod {setting} ok" in r.stdout
        lines = [ln.split() for ln in r.stdout.splitlines()]
        out[setting] = {(ln[0], ln[1], ln[2]): ln[3] for ln in lines if ln and ln[0] in ("TREE", "BIGTREE", "PROOF")}
    return out


@pytest.fixture(scope="module")
def expected():
    """the definition's digests, computed once: {("PROOF", field id, key): ..} and {("TREE", field id, key): ..}"""
    out = {}
    for case in ref.GPU_CASES:
        fi, table, shift, seed = ref.case_inputs(case, worst_case_values)
        product, proof, point, claim = ref.prove(fi, table, seed, shift)
        assert ref.verify(fi, case[0], seed, product, proof, shift) == (point, claim), case   # the same bytes as the device's, below
        out[("PROOF", FIELD_IDS[fi], case_key(case))] = digest(orc.from_int(fi, product).tobytes() + proof + orc.from_ints(fi, point).tobytes()
                                                               + orc.from_int(fi, claim).tobytes())
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for n in ref.TREE_VARS:
            table = tree_case(fi, n, p)
            for name, shift in (("null", None), ("minus_one", p - 1)):
                out[("TREE", FIELD_IDS[fi], "n%d_%s" % (n, name))] = digest(orc.from_ints(field, ref.product_tree(table, shift, p)).tobytes())
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_proof_on_every_setting(children, expected, setting):
    """product, proof, point and claim of zk_gprod_prove against gprod_ref.prove, byte for byte, with 1, 2 and 3 levels of the tree per
    launch and by default; zk_gprod_verify_host accepted each in the child (with the prover's point and claim), gprod_ref.verify in the
    fixture.  The extras take 1, 2, 3 and 4 levels above the LDS stage: every arity of the fused kernel, and two launches"""
    want = {key: dg for key, dg in expected.items() if key[0] == "PROOF"}
    got = {key: dg for key, dg in children[setting].items() if key[0] == "PROOF"}
    assert len(want) == len(ref.GPU_CASES) and set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, (setting, wrong[:20], len(wrong))


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_trees_against_python_integers(children, expected, setting):
    """zk_mle_product_tree on all three fields at every size from n = 1 to two past the LDS stage, shift NULL and p - 1"""
    want = {key: dg for key, dg in expected.items() if key[0] == "TREE"}
    got = {key: dg for key, dg in children[setting].items() if key[0] == "TREE"}
    assert len(want) == 3 * 2 * len(ref.TREE_VARS) and set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, (setting, wrong)


@pytest.fixture(scope="module")
def oracle_heaps():
    """{n: digest of the C oracle's heap over its generator's table}, one per size, shared by the settings"""
    sizes = sorted({n for setting in SETTINGS for n in big_vars(setting)})
    return {n: digest(oracle_heap(orc, FIELDS[0], orc.fill_random(FIELDS[0], BIG_SEED + n, 1 << n)).tobytes()) for n in sizes}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_trees_against_the_oracle(children, oracle_heaps, setting):
    """BN254 at 2^20 elements on every setting: every level of the heap against repeated orc.prod_reduce of the halves.  With one level
    per launch also 2^24, the smallest table at which the grid cap of 2^14 workgroups makes a wave take a second run; on the default
    route that happens from 2^26 on (gprod_ref.SECOND_TRIP_VARS), not below 2^25, so there is no such table to run"""
    sizes = big_vars(setting)
    assert sizes == ((BIG_VARS, 24) if setting == "fuse1" else (BIG_VARS,)) and ref.SECOND_TRIP_VARS[ref.FUSE_DEFAULT] > 25
    got = {key: dg for key, dg in children[setting].items() if key[0] == "BIGTREE"}
    assert set(got) == {("BIGTREE", FIELD_IDS[0], "n%d" % n) for n in sizes}
    for n in sizes:
        assert got[("BIGTREE", FIELD_IDS[0], "n%d" % n)] == oracle_heaps[n], (setting, n)


def test_one_proof_on_the_workloads_scale(oracle_heaps):
    """BN254, n = 20, on orc.fill_random's table, which zk_mle_fill_random makes on the device: the chained big rounds exist only above
    the finisher sizes.  zk_gprod_verify_host accepts; the definition's verifier (O(n^2)) accepts with the same point and claim; the
    product is the oracle's; the claim that is left is the oracle's evaluation of the table"""
    field, n = FIELDS[0], BIG_VARS
    ctx = zk_amd.Context(field, 0)
    t = MLE.random(ctx, n, BIG_SEED + n)
    seed = bytes(range(32))
    product, proof, point, claim = zk_amd.grand_product_prove(t, seed)
    got = zk_amd.grand_product_verify(field, n, seed, product, proof)
    assert got is not None and np.array_equal(got[0], point) and np.array_equal(got[1], claim)
    want = ref.verify(field, n, seed, orc.to_int(field, product), proof)
    assert want is not None and want[0] == orc.to_ints(field, point) and want[1] == orc.to_int(field, claim)
    table = orc.fill_random(field, BIG_SEED + n, 1 << n)
    heap = oracle_heap(orc, field, table)
    assert digest(heap.tobytes()) == oracle_heaps[n] and np.array_equal(heap[1], product)
    assert np.array_equal(orc.mle_evaluate(field, n, table, point), claim)
    assert np.array_equal(t.evaluation_slice(), table)   # t is bit-identical after the proof
    t.free()
    ctx.close()


@pytest.fixture(params=range(3), ids=FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def test_repeated_calls_over_stale_pool_blocks(fctx):
    """two calls give identical bytes after random tables of the scratch's size classes have been allocated and freed, and t is
    bit-identical after tree and proof"""
    fi, field, ctx = fctx
    p = orc.modulus(field)
    n = 12
    src = orc.from_ints(field, tree_case(fi, n, p))
    shift = orc.from_int(field, 3)
    t = MLE.new(ctx, n, src)
    first = zk_amd.grand_product_prove(t, bytes(32), shift)
    heap = zk_amd.product_tree(t, shift)
    first_heap = heap.evaluation_slice().copy()
    heap.free()
    for n_vars in list(range(0, 14)) * 2:
        MLE.random(ctx, n_vars, 31 + n_vars).free()
    again = zk_amd.grand_product_prove(t, bytes(32), shift)
    assert first[1] == again[1] and all(np.array_equal(a, b) for a, b in zip(first[::2], again[::2])) and np.array_equal(first[3], again[3])
    heap = zk_amd.product_tree(t, shift)
    assert np.array_equal(heap.evaluation_slice(), first_heap) and np.array_equal(first_heap[1], first[0])
    heap.free()
    assert np.array_equal(t.evaluation_slice(), src)
    table = orc.to_ints(field, src)
    assert (orc.to_int(field, first[0]), first[1]) == ref.prove(field, table, bytes(32), 3)[:2]


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    n = 6
    t, t_other, t0 = MLE.random(ctx, n, 1), MLE.random(other, n, 1), MLE.random(ctx, 0, 2)
    before = t.evaluation_slice().copy()
    raw_p = np.frombuffer(p.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    pp = raw_p.ctypes.data_as(u64p)
    h = c.c_void_p()
    tr = lib.zk_mle_product_tree
    # NULL, another context, n, the shift -- in this order
    assert tr(None, t._h, None, c.byref(h)) == BAD and tr(ctx._h, None, None, c.byref(h)) == BAD and tr(ctx._h, t._h, None, None) == BAD
    assert tr(ctx._h, t_other._h, pp, c.byref(h)) == MISMATCH and tr(other._h, t._h, None, c.byref(h)) == MISMATCH
    assert tr(ctx._h, t0._h, pp, c.byref(h)) == BAD and tr(ctx._h, t._h, pp, c.byref(h)) == BAD
    assert not h.value
    seed = np.arange(32, dtype=np.uint8)
    sp = seed.ctypes.data_as(u8p)
    buf = np.full(ref.proof_bytes(n), 7, dtype=np.uint8)
    prod, point, claim = (np.full(s, 9, dtype=np.uint64) for s in (4, 4 * n, 4))
    bp, qp, zp, cp = buf.ctypes.data_as(u8p), prod.ctypes.data_as(u64p), point.ctypes.data_as(u64p), claim.ctypes.data_as(u64p)
    pv = lib.zk_gprod_prove
    good = [ctx._h, t._h, None, sp, qp, bp, zp, cp]
    for i in (0, 1, 3, 4, 5, 6, 7):   # every pointer but the shift
        bad = list(good)
        bad[i] = None
        assert pv(*bad) == BAD, i
    assert pv(other._h, t._h, pp, sp, qp, bp, zp, cp) == MISMATCH and pv(ctx._h, t_other._h, None, sp, qp, bp, zp, cp) == MISMATCH
    assert pv(ctx._h, t0._h, pp, sp, qp, bp, zp, cp) == BAD                         # n = 0 before the shift
    assert pv(ctx._h, t._h, pp, sp, qp, bp, zp, cp) == BAD                          # a shift that is not reduced
    assert (buf == 7).all() and (prod == 9).all() and (point == 9).all() and (claim == 9).all()   # nothing was written by any of them
    assert pv(*good) == 0
    table = orc.to_ints(field, before)
    want = ref.prove(field, table, seed.tobytes())
    assert (orc.to_int(field, prod), buf.tobytes(), orc.to_ints(field, point.reshape(n, 4)), orc.to_int(field, claim)) == want
    # the measurement hook gives a time on its three paths and leaves the table alone
    ms = c.c_double(-1.0)
    for path in (0, 1, 2):
        ms.value = -1.0
        assert lib.zk_bench_gprod(ctx._h, t._h, path, 2, c.byref(ms)) == 0 and ms.value > 0, path
    assert zk_amd.bench_gprod(t, path=2, reps=1) > 0
    ms.value = -1.0
    assert lib.zk_bench_gprod(ctx._h, t._h, 3, 1, c.byref(ms)) == BAD and lib.zk_bench_gprod(ctx._h, t._h, 0, 0, c.byref(ms)) == BAD
    assert lib.zk_bench_gprod(ctx._h, t._h, 0, 1, None) == BAD and lib.zk_bench_gprod(ctx._h, None, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_gprod(other._h, t._h, 0, 1, c.byref(ms)) == MISMATCH and lib.zk_bench_gprod(ctx._h, t0._h, 0, 1, c.byref(ms)) == BAD
    assert ms.value == -1.0 and np.array_equal(t.evaluation_slice(), before)
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_gprod.cpp over zk.hpp: trees, proofs, the verifier's verdicts, NULL and zero shifts, the errors"""
    exe = str(tmp_path / "test_gprod")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_gprod.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: gprod host tests passed" in r.stdout


def test_permutation_check_from_public_calls():
    """b is a permutation of a: both are committed, gamma is drawn from a transcript over the two roots, the two grand products with
    shift gamma are equal, and the claims the two proofs leave are opened from the commitments at the returned points.  With one entry
    of b changed the products differ"""
    field, n, blowup, log_final, queries = zk_amd.BN254_FR, 6, 1, 0, 8
    p = orc.modulus(field)
    ctx = zk_amd.Context(field, 0)
    rng = np.random.default_rng(5)
    a = [int(x) for x in rng.integers(1, 1 << 62, 1 << n)]
    b = [a[i] for i in rng.permutation(1 << n)]
    one = orc.from_int(field, 1)

    def run(values_a, values_b):
        tabs = [MLE.new(ctx, n, orc.from_ints(field, v)) for v in (values_a, values_b)]
        coms = [zk_amd.MultilinearCommitment.commit(t, blowup, one) for t in tabs]
        roots = [com.root() for com in coms]
        tr = zk_amd.Transcript()
        tr.append(roots[0] + roots[1])
        gamma = tr.sample_field_element(field)        # after both commitments
        seed = zk_amd.keccak256(roots[0] + roots[1])  # binds both tables
        products = []
        for t, com, root in zip(tabs, coms, roots):
            product, proof, point, claim = zk_amd.grand_product_prove(t, seed, gamma)
            # the verifier: the argument, then the claim it leaves against the commitment
            got = zk_amd.grand_product_verify(field, n, seed, product, proof, gamma)
            assert got is not None and np.array_equal(got[0], point) and np.array_equal(got[1], claim)
            value, opening = com.open(got[0], log_final, queries, seed)
            assert np.array_equal(value, got[1])
            assert zk_amd.mlpcs_verify(field, root, got[0], got[1], opening, blowup, log_final, queries, one, seed)
            products.append(orc.to_int(field, product))
        for x in tabs + coms:
            x.free()
        return products, orc.to_int(field, gamma)

    (pa, pb), gamma = run(a, b)
    want = 1
    for x in a:
        want = want * (x + gamma) % p
    assert pa == pb == want
    b[17] = (b[17] + 1) % p
    (pa, pb), gamma = run(a, b)
    assert pa != pb
    ctx.close()
