"""zk_deep_quotient / zk_pcs_commit / zk_pcs_open / zk_pcs_verify_host / zk_bench_deep_quotient on the device.  The reference has no
polynomial commitment: tests/pcs_ref.py is the definition.  In child processes under ZK_FRI_FUSED_FOLD (the only switch on the path):
every opening of the shared case list -- root, values and proof -- byte for byte against the definition, on every setting; in the default
child every quotient (a single output pair, a partial wave, one and two waves, exactly one chunk, two chunks = the split of the power
table, more; 1 to 17 columns; z and alpha in {0, 1, p - 1, random}; shifts 1, 5, p - 1; worst-case limb patterns).  In the parent two
openings of one handle, the error table, the measurement hook and the C++ mirror.

No case for a capped grid: the quotient's launches take one workgroup per chunk of 2^11 outputs and no loop (pcs.hip quotient_launch), so
every output has exactly one writer at every size and no allocatable size wraps; a grid past 2^31 - 1 chunks (2^42 outputs) is refused."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import UnivariatePolynomial as Poly
from zk_amd._lib import c, lib, u8p, u64p, vpp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_ref  # noqa: E402
import pcs_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from pcs_check import SETTINGS, SWITCH, case_key, digest, quotient_key  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "pcs_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
NO_ROOT, BAD, MISMATCH = -7, -20, -26


@pytest.fixture(scope="module")
def children():
    """{setting: {(kind, field id, key): digest}}: one child process per switch setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"pcs {setting} ok" in r.stdout
        lines = [ln.split() for ln in r.stdout.splitlines()]
        out[setting] = {(ln[0], ln[1], ln[2]): ln[3] for ln in lines if ln and ln[0] in ("QUO", "PROOF")}
    return out


@pytest.fixture(scope="module")
def expected_quotients():
    """{("QUO", field id, key): digest} from the definition, computed once"""
    out = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for log_n, k in ref.quotient_sizes(fi):
            cols = ref.quotient_columns(p, fi, log_n, k, worst_case_values)
            for shift_name, zi, ai in ref.quotient_combos(log_n, k):
                s, z, alpha, ys = ref.quotient_case(fi, log_n, k, shift_name, zi, ai)
                want = ref.quotient(field, cols, s, z, ys, alpha)
                out[("QUO", fri_ref.FIELD_IDS[fi], quotient_key(log_n, k, shift_name, zi, ai))] = digest(orc.from_ints(field, want).tobytes())
    return out


@pytest.fixture(scope="module")
def expected_proofs():
    """{("PROOF", field id, key): digest of root + values + proof} from the definition, which also accepts each of them"""
    out = {}
    for case in ref.GPU_CASES:
        k, d, b, a, f, q = case
        fi = ref.case_field(case)
        polys, shift, seed, z = ref.case_inputs(fi, case)
        committed = ref.commit(fi, polys, d, b, a, shift)
        root = ref.merkle_ref.root(committed[2])
        ys, proof = ref.prove(fi, polys, d, b, a, f, q, shift, seed, z, committed=committed)
        assert ys == [ref.evaluate(fi, co, z) for co in polys]
        assert ref.verify(fi, k, d, b, a, f, q, shift, seed, root, z, ys, proof), case   # the same bytes as the device's, below
        out[("PROOF", fri_ref.FIELD_IDS[fi], case_key(case))] = digest(root + orc.from_ints(fi, ys).tobytes() + proof)
    return out


def test_every_quotient_against_the_definition(children, expected_quotients):
    """zk_deep_quotient against pcs_ref.quotient, byte for byte; the other children run no quotient (no switch reaches it)"""
    got = {key: dg for key, dg in children["default"].items() if key[0] == "QUO"}
    for fi in range(3):   # thinned, but every size and every number of columns is there
        sizes = ref.quotient_sizes(fi)
        assert {n for n, _ in sizes} == set(ref.QUOTIENT_LOGS) and len(set(sizes)) == len(sizes)
    assert {k for _, k in ref.quotient_sizes(0)} == set(ref.QUOTIENT_COLUMNS) and {(12, k) for k in ref.QUOTIENT_COLUMNS} <= set(ref.quotient_sizes(0))
    assert len(expected_quotients) == sum(len(ref.quotient_combos(n, k)) for fi in range(3) for n, k in ref.quotient_sizes(fi))
    assert set(got) == set(expected_quotients)
    wrong = sorted(key for key, want in expected_quotients.items() if got[key] != want)
    assert not wrong, (wrong[:20], len(wrong))
    assert not any(key[0] == "QUO" for setting in ("fused", "binary") for key in children[setting])


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_opening_on_every_setting(children, expected_proofs, setting):
    """root, values (= f_c(z)) and proof of zk_pcs_commit / zk_pcs_open against pcs_ref.prove, byte for byte, with the fused fold kernel,
    with the binary launches and by default; zk_pcs_verify_host accepted each in the child, pcs_ref.verify the same bytes in the fixture"""
    got = {key: dg for key, dg in children[setting].items() if key[0] == "PROOF"}
    assert len(expected_proofs) == len(ref.GPU_CASES) and set(got) == set(expected_proofs)
    wrong = sorted(key for key, want in expected_proofs.items() if got[key] != want)
    assert not wrong, (setting, wrong[:20], len(wrong))


@pytest.fixture(params=range(3), ids=fri_ref.FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def test_two_openings_of_one_handle(fctx):
    """the handle survives an open: a second opening at another z (and the first again) gives the definition's bytes, the root unchanged;
    the polynomials may be freed after the commitment; zk_deep_quotient through its wrapper into a table of the caller's"""
    fi, field, ctx = fctx
    p = orc.modulus(field)
    case = (2, 8, 2, 3, 2, 8)
    k, d, b, a, f, q = case
    polys, shift, seed, z1 = ref.case_inputs(fi, case)
    sv = orc.from_int(field, shift)
    MLE.random(ctx, 13, 77).free()   # the tables of the commitment are cut from stale data, not zeros
    handles = [Poly.new(ctx, orc.from_ints(field, co)) for co in polys]
    com = zk_amd.PolyCommitment.commit(handles, d, b, a, sv)
    for h in handles:
        h.free()
    assert com.n_polys() == k
    committed = ref.commit(field, polys, d, b, a, shift)
    root = com.root()
    assert root == ref.merkle_ref.root(committed[2])
    z2 = (z1 * 7 + 3) % p
    while ref.on_domain(field, d + b, shift, z2):
        z2 = (z2 + 1) % p
    for z in (z1, z2, z1):
        values, proof = com.open(orc.from_int(field, z), f, q, seed)
        ys, want = ref.prove(field, polys, d, b, a, f, q, shift, seed, z, committed=committed)
        assert orc.to_ints(field, values) == ys and proof == want and len(proof) == zk_amd.pcs_proof_bytes(*case), z
        assert zk_amd.pcs_verify(field, root, orc.from_int(field, z), values, proof, d, b, a, f, q, sv, seed)
        zb = (z + 1) % p
        while ref.on_domain(field, d + b, shift, zb):
            zb = (zb + 1) % p
        assert not zk_amd.pcs_verify(field, root, orc.from_int(field, zb), values, proof, d, b, a, f, q, sv, seed)
    assert com.root() == root
    # another final length and query count on the same handle
    values, proof = com.open(orc.from_int(field, z2), 5, 3, seed)
    assert (orc.to_ints(field, values), proof) == ref.prove(field, polys, d, b, a, 5, 3, shift, seed, z2, committed=committed)
    com.free()
    cols_int = ref.quotient_columns(p, fi, 9, 2, worst_case_values)
    cols = [MLE.new(ctx, 9, orc.from_ints(field, col)) for col in cols_int]
    out = MLE.random(ctx, 9, 5)
    ys = [3, p - 1]
    while ref.on_domain(field, 9, shift, z2):
        z2 = (z2 + 1) % p
    assert zk_amd.deep_quotient(cols, sv, orc.from_int(field, z2), orc.from_ints(field, ys), orc.from_int(field, 7), out) is out
    assert orc.to_ints(field, out.evaluation_slice()) == ref.quotient(field, cols_int, shift, z2, ys, 7)


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    n = 10
    col0, col1, out, small = MLE.random(ctx, n, 1), MLE.random(ctx, n, 2), MLE.random(ctx, n, 3), MLE.random(ctx, n - 1, 4)
    col_other, out_other = MLE.random(other, n, 1), MLE.random(other, n, 3)
    before, before_out = col0.evaluation_slice().copy(), out.evaluation_slice().copy()
    five, zero, two = orc.from_int(field, 5), np.zeros(4, dtype=np.uint64), orc.from_ints(field, [2, 3])
    raw_p = np.frombuffer(p.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    on = orc.from_int(field, 5 * pow(fri_ref.root(field, 1 << n), 5, p) % p)   # z = s w^5
    fp, zp, pp, op, yp = (x.ctypes.data_as(u64p) for x in (five, zero, raw_p, on, two))
    ms = c.c_double(-1.0)

    def ptrs(*tables):
        arr = (c.c_void_p * len(tables))(*[t._h for t in tables])
        return c.cast(arr, vpp), arr

    cols, _k1 = ptrs(col0, col1)
    single, _k0 = ptrs(col0)
    mixed, _k2 = ptrs(col0, col_other)
    uneven, _k3 = ptrs(col0, small)
    aliased, _k4 = ptrs(col0, out)
    q = lib.zk_deep_quotient
    # NULL, another context, the shapes, the elements, the domain -- in this order
    assert q(ctx._h, cols, 2, None, zp, yp, fp, out._h) == BAD
    assert q(ctx._h, mixed, 0, fp, zp, yp, fp, out._h) == BAD                      # n_columns == 0 before the contexts
    assert q(ctx._h, mixed, 2, fp, zp, yp, fp, out._h) == MISMATCH
    assert q(ctx._h, cols, 2, fp, zp, yp, fp, out_other._h) == MISMATCH
    assert q(other._h, cols, 2, fp, zp, yp, fp, out._h) == MISMATCH
    assert q(ctx._h, uneven, 2, fp, zp, yp, fp, out._h) == BAD                     # columns of differing sizes
    assert q(ctx._h, cols, 2, fp, zp, yp, fp, small._h) == BAD                     # out of the wrong size
    assert q(ctx._h, aliased, 2, fp, zp, yp, fp, out._h) == BAD                    # out is one of the columns
    assert q(ctx._h, cols, 2, zp, zp, yp, fp, out._h) == BAD                       # shift = 0
    for where in range(4):                                                        # shift, z, a value, alpha not fully reduced
        args = [fp, zp, yp, fp]
        args[where] = pp
        assert q(ctx._h, cols, 2, *args, out._h) == BAD, where
    assert q(ctx._h, cols, 2, fp, op, yp, fp, out._h) == BAD                       # z = s w^5 is on the domain
    assert q(ctx._h, cols, 2, fp, fp, yp, fp, out._h) == BAD                       # and so is s itself
    assert np.array_equal(out.evaluation_slice(), before_out) and np.array_equal(col0.evaluation_slice(), before)
    assert q(ctx._h, cols, 2, fp, zp, yp, zp, out._h) == 0                         # z = 0 and alpha = 0 are values like any other
    want = ref.quotient(field, [orc.to_ints(field, col0.evaluation_slice()), orc.to_ints(field, col1.evaluation_slice())], 5, 0, [2, 3], 0)
    assert orc.to_ints(field, out.evaluation_slice()) == want
    # commit and open
    poly = Poly.new(ctx, orc.from_ints(field, list(range(1, 17))))
    poly_other = Poly.new(other, orc.from_ints(field, list(range(1, 17))))
    h = c.c_void_p()

    def polys_of(*ps):
        arr = (c.c_void_p * len(ps))(*[x._h for x in ps])
        return c.cast(arr, vpp), arr

    one_poly, _k5 = polys_of(poly)
    mixed_polys, _k6 = polys_of(poly, poly_other)
    cm = lib.zk_pcs_commit
    assert cm(ctx._h, mixed_polys, 2, 4, 2, 2, fp, c.byref(h)) == MISMATCH and cm(other._h, one_poly, 1, 4, 2, 2, fp, c.byref(h)) == MISMATCH
    for bad in ((4, 2, 0), (4, 2, 4), (4, 0, 2), (4, 9, 2), (3, 2, 1), (2, 2, 3), (41, 2, 1)):   # (3, 2, 1): 16 coefficients against a bound of 8
        assert cm(ctx._h, one_poly, 1, *bad, fp, c.byref(h)) == BAD, bad
    many = (c.c_void_p * 129)(*([poly._h] * 129))
    assert cm(ctx._h, c.cast(many, vpp), 129, 4, 2, 3, fp, c.byref(h)) == BAD      # 129 * 8 columns
    assert cm(ctx._h, one_poly, 1, 4, 2, 2, zp, c.byref(h)) == BAD and cm(ctx._h, one_poly, 1, 4, 2, 2, pp, c.byref(h)) == BAD
    assert cm(ctx._h, one_poly, 1, 27, 2, 3, fp, c.byref(h)) == NO_ROOT            # BN254: two-adicity 28
    assert not h.value
    com = zk_amd.PolyCommitment.commit([poly], 4, 2, 2, five)
    seed = np.arange(32, dtype=np.uint8)
    sp = seed.ctypes.data_as(u8p)
    buf = np.full(ref.proof_bytes(1, 4, 2, 2, 0, 8), 7, dtype=np.uint8)
    vals = np.full(4, 9, dtype=np.uint64)
    bp, vp = buf.ctypes.data_as(u8p), vals.ctypes.data_as(u64p)
    opn = lib.zk_pcs_open
    assert opn(other._h, com._h, zp, 0, 8, sp, vp, bp) == MISMATCH
    for f, nq in ((4, 8), (1, 8), (0, 0), (0, 1025)):
        assert opn(ctx._h, com._h, zp, f, nq, sp, vp, bp) == BAD, (f, nq)
    on6 = orc.from_int(field, 5 * pow(fri_ref.root(field, 1 << 6), 5, p) % p)
    assert opn(ctx._h, com._h, on6.ctypes.data_as(u64p), 0, 8, sp, vp, bp) == BAD and opn(ctx._h, com._h, pp, 0, 8, sp, vp, bp) == BAD
    root_buf = np.zeros(32, dtype=np.uint8)
    assert lib.zk_pcs_root(other._h, com._h, root_buf.ctypes.data_as(u8p)) == MISMATCH
    assert (buf == 7).all() and (vals == 9).all()                                 # nothing was written by any of them
    assert opn(ctx._h, com._h, zp, 0, 8, sp, vp, bp) == 0
    ys, want = ref.prove(field, [list(range(1, 17))], 4, 2, 2, 0, 8, 5, seed.tobytes(), 0)
    assert buf.tobytes() == want and orc.to_ints(field, vals.reshape(1, 4)) == ys == [1]
    # the measurement hook gives a time and leaves the columns alone
    for width, columns in ((1, single), (2, cols)):
        ms.value = -1.0
        assert lib.zk_bench_deep_quotient(ctx._h, columns, width, out._h, 2, c.byref(ms)) == 0 and ms.value > 0, width
    assert zk_amd.bench_deep_quotient([col0, col1], out, reps=1) > 0
    ms.value = -1.0
    assert lib.zk_bench_deep_quotient(ctx._h, cols, 2, out._h, 0, c.byref(ms)) == BAD
    assert lib.zk_bench_deep_quotient(ctx._h, mixed, 2, out._h, 1, c.byref(ms)) == MISMATCH
    assert lib.zk_bench_deep_quotient(ctx._h, cols, 2, small._h, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_deep_quotient(ctx._h, aliased, 2, out._h, 1, c.byref(ms)) == BAD
    assert ms.value == -1.0 and np.array_equal(col0.evaluation_slice(), before)
    com.free()
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_pcs.cpp over zk.hpp: openings, the verifier's verdicts, two openings of one commitment, the quotient, the errors"""
    exe = str(tmp_path / "test_pcs")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_pcs.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: pcs host tests passed" in r.stdout
