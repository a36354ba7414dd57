"""zk_fri_lde / zk_fri_fold / zk_fri_prove / zk_fri_verify_host / zk_bench_fri_fold on the device.  The reference has no FRI:
tests/fri_ref.py is the definition.  The fused fold kernel, the binary launches and the default in child processes under
ZK_FRI_FUSED_FOLD: every fold (each arity at a single output, a partial wave, one and several workgroups and both sides of the split of the
two-level power table at 2^12, shifts 1, 5, p - 1, beta in {0, 1, p - 1, random}, worst-case limb patterns) and every proof of the shared
case list byte for byte against the definition; in the parent the LDE, the wrappers, the error table, the measurement hook and the C++
mirror.  In the same child processes the sizes at which loops take more than one trip: folds with 2^24 outputs (k_fri_fold's grid is
capped at 2^23) and proofs whose first trees have 2^21 rows."""
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
from zk_amd._lib import c, lib, u8p, u64p

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from fri_check import SETTINGS, SWITCH, big_fold_key, case_key, digest, fold_key  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "fri_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
EVAL_LEN, NO_ROOT, BAD, MISMATCH = -1, -7, -20, -26


@pytest.fixture(scope="module")
def child_lines():
    """{setting: the split lines of the child's output}: one child process per switch setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"fri {setting} ok" in r.stdout
        out[setting] = [ln.split() for ln in r.stdout.splitlines()]
    return out


@pytest.fixture(scope="module")
def children(child_lines):
    """{setting: {(kind, field id, key): digest}}"""
    return {setting: {(ln[0], ln[1], ln[2]): ln[3] for ln in lines if ln and ln[0] in ("FOLD", "PROOF")} for setting, lines in child_lines.items()}


@pytest.fixture(scope="module")
def big_children(child_lines):
    """{setting: ({(case key, check): the rest of its BIG line}, {case key: digest of the large proof})}"""
    return {setting: ({(ln[1], ln[2]): ln[3:] for ln in lines if ln and ln[0] == "BIG"}, {ln[1]: ln[2] for ln in lines if ln and ln[0] == "BIGPROOF"})
            for setting, lines in child_lines.items()}


@pytest.fixture(scope="module")
def expected():
    """{(kind, field id, key): digest} from the definition, computed once"""
    out = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for a, log_n in ref.fold_cases(fi):
            v = ref.fold_input(p, fi, log_n, worst_case_values)
            betas = ref.fold_betas(p, fi, a, log_n)
            for shift_name, k in ref.fold_combos(log_n):
                want = ref.fold(field, v, ref.shift_value(p, shift_name), betas[k], a)
                out[("FOLD", ref.FIELD_IDS[fi], fold_key(a, log_n, shift_name, k))] = digest(orc.from_ints(field, want).tobytes())
    for case in ref.GPU_CASES:
        fi = ref.case_field(case)
        coeffs, shift, seed = ref.case_inputs(fi, case)
        out[("PROOF", ref.FIELD_IDS[fi], case_key(case))] = digest(ref.prove(fi, coeffs, *case, shift, seed))
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_fold_and_every_proof_on_every_path(children, expected, setting):
    """zk_fri_fold against fri_ref.fold and zk_fri_prove against fri_ref.prove, byte for byte, with the fused kernel, with the binary
    launches and by default; both paths therefore give identical bytes"""
    got = children[setting]
    n_folds = sum(len(ref.fold_combos(n)) for fi in range(3) for _, n in ref.fold_cases(fi))
    assert len(expected) == n_folds + len(ref.GPU_CASES) and set(got) == set(expected)
    wrong = sorted(key for key, want in expected.items() if got[key] != want)
    assert not wrong, (setting, wrong[:20], len(wrong))
    assert children["fused"] == children["binary"]


BIG_FOLD_CHECKS = ("even_odd", "input_intact", "sampled", "half_even_sampled", "half_odd_sampled", "completed")
BIG_PROOF_CHECKS = ("length", "host_verifier_accepts", "definition_accepts", "flipped_byte_rejected", "wrong_seed_rejected",
                    "first_root_is_the_commitment_to_the_lde", "first_root_is_the_reference_root_of_the_lde", "completed")


@pytest.mark.parametrize("setting", ["fused", "binary"])
def test_folds_with_more_outputs_than_one_sweep(big_children, setting):
    """zk_fri_fold with M = 2^24 outputs, BN254, a seeded random table, shift and beta: fri.hip caps k_fri_fold<a, true> at 2^15 workgroups
    of 256 outputs, so the second half of the outputs comes from the loop's second trip.  2^25 points by 2 with the fused kernel and with
    the binary launches (the same kernel there); 2^27 points by 8 (4 GiB in) with the fused kernel only.  Per fold: 4096 outputs (0, 63,
    64, M - 1, 64 on either side of 2^23, seeded ones) against fri_ref.fold_at on the downloaded input; on the device, the whole output
    against the interleaved folds of the even inputs (shift s) and of the odd inputs (shift s w_N), which have 2^23 outputs and do not
    wrap; 256 outputs of each of those against fold_at; the input left intact."""
    checks, _ = big_children[setting]
    cases = [big_fold_key(a, log_n) for a, log_n, settings in ref.FOLD_BIG if setting in settings]
    assert cases and len(cases) == (2 if setting == "fused" else 1)
    assert {key for key in checks if key[0].startswith("fold_")} == {(case, name) for case in cases for name in BIG_FOLD_CHECKS}
    failed = sorted((key, rest) for key, rest in checks.items() if key[0] in cases and rest[0] != "PASS")
    assert not failed, (setting, failed)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_proofs_whose_first_tree_wraps(big_children, setting):
    """d = 21, b = 1, Q = 8, f = 0, BN254, a = 1 and a = 3: layer 0 has 2^22 points, and at a = 1 its tree has 2^21 rows, so that
    k_merkle_leaves and k_merkle_level take several trips inside zk_fri_prove (at a = 3 the tree has 2^19 rows: exactly one trip).
    zk_amd.fri_verify and fri_ref.verify accept; a flipped byte and another seed are rejected by both; the first root is
    MerkleTree.commit over the 2^a contiguous column views of zk_amd.fri_lde, and merkle_ref.commit_bulk's root over the downloaded LDE
    (the first runs the prover's own kernels again); the bytes are the same with the fused kernel, with the binary launches and by
    default.  Acceptance pins the queried positions only: the large folds and the large trees of
    tests/test_gpu_merkle.py pin the rest.  There is no byte-for-byte reference (fri_ref.prove would take minutes at this size)."""
    checks, digests = big_children[setting]
    cases = [case_key(case) for case in ref.PROOF_BIG]
    assert {key for key in checks if not key[0].startswith("fold_")} == {(case, name) for case in cases for name in BIG_PROOF_CHECKS}
    failed = sorted((key, rest) for key, rest in checks.items() if key[0] in cases and rest[0] != "PASS")
    assert not failed, (setting, failed)
    assert set(digests) == set(cases)
    assert digests == big_children["fused"][1] == big_children["binary"][1] == big_children["default"][1]


@pytest.fixture(params=range(3), ids=ref.FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def test_lde_against_the_definition(fctx):
    """0, 1, 2^d - 1 and 2^d coefficients at blowups 1, 2 and 8 and below / above the NTT's small-size path; the polynomial is left intact"""
    fi, field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(0x1DE + fi)
    for d, b in ((0, 1), (1, 1), (3, 2), (6, 1), (7, 1), (9, 3), (12, 1)):
        for length in sorted({0, 1, (1 << d) - 1, 1 << d}):
            coeffs = [rng.randrange(p) for _ in range(length)]
            if length:
                coeffs[-1] = p - 1
            src = orc.from_ints(field, coeffs)
            poly = Poly.new(ctx, src)
            for shift in (1, 5, p - 1):
                got = zk_amd.fri_lde(poly, d + b, orc.from_int(field, shift))
                assert got.n_vars() == d + b
                assert orc.to_ints(field, got.evaluation_slice()) == ref.lde(field, coeffs, d + b, shift), (d, b, length, shift)
                got.free()
            assert np.array_equal(poly.coefficients(), src)
            poly.free()


def test_wrappers_prove_and_verify(fctx):
    fi, field, ctx = fctx
    p = orc.modulus(field)
    case = (8, 2, 3, 2, 8)
    coeffs, shift, seed = ref.case_inputs(fi, case)
    sv = orc.from_int(field, shift)
    big = MLE.random(ctx, 13, 77)   # the layers of the proof are cut from stale data, not zeros
    big.free()
    poly = Poly.new(ctx, orc.from_ints(field, coeffs))
    proof = zk_amd.fri_prove(poly, *case, sv, seed)
    assert len(proof) == zk_amd.fri_proof_bytes(*case) == ref.proof_bytes(*case)
    assert proof == ref.prove(field, coeffs, *case, shift, seed)
    assert zk_amd.fri_prove(poly, *case, sv, seed) == proof
    assert zk_amd.fri_verify(field, proof, *case, sv, seed)
    flipped = bytearray(proof)
    flipped[len(proof) // 3] ^= 2
    assert not zk_amd.fri_verify(field, bytes(flipped), *case, sv, seed)
    assert not zk_amd.fri_verify(field, proof, *case, sv, bytes(32))
    assert np.array_equal(poly.coefficients(), orc.from_ints(field, coeffs))
    # fewer coefficients than the bound, the empty polynomial included
    for length in (0, 1, 100):
        short = Poly.new(ctx, orc.from_ints(field, coeffs[:length]))
        got = zk_amd.fri_prove(short, *case, sv, seed)
        assert got == ref.prove(field, coeffs[:length], *case, shift, seed) and zk_amd.fri_verify(field, got, *case, sv, seed), length
    # fold through the wrapper, into a table of the caller's
    v = ref.fold_input(p, fi, 10, worst_case_values)
    layer = MLE.new(ctx, 10, orc.from_ints(field, v))
    out = MLE.random(ctx, 8, 5)
    assert zk_amd.fri_fold(layer, 2, sv, orc.from_int(field, 7), out) is out
    assert orc.to_ints(field, out.evaluation_slice()) == ref.fold(field, v, shift, 7, 2)


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    layer, out1, out3, tiny = MLE.random(ctx, 10, 1), MLE.random(ctx, 9, 2), MLE.random(ctx, 7, 3), MLE.random(ctx, 1, 4)
    layer_other, out_other = MLE.random(other, 10, 1), MLE.random(other, 9, 2)
    poly = Poly.new(ctx, orc.from_ints(field, list(range(1, 17))))
    poly_other = Poly.new(other, orc.from_ints(field, list(range(1, 17))))
    before = layer.evaluation_slice().copy()
    five, zero = orc.from_int(field, 5), np.zeros(4, dtype=np.uint64)
    raw_p = np.frombuffer(p.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    fp, zp, pp = five.ctypes.data_as(u64p), zero.ctypes.data_as(u64p), raw_p.ctypes.data_as(u64p)
    h, ms = c.c_void_p(), c.c_double(-1.0)
    # zk_fri_fold: NULL, another context, the arity, the shift and beta, the output, the domain, the length -- in this order
    assert lib.zk_fri_fold(None, layer._h, 1, fp, fp, out1._h) == BAD
    assert lib.zk_fri_fold(ctx._h, layer._h, 1, None, fp, out1._h) == BAD
    assert lib.zk_fri_fold(ctx._h, layer_other._h, 0, fp, fp, out1._h) == MISMATCH     # before the arity
    assert lib.zk_fri_fold(ctx._h, layer._h, 1, fp, fp, out_other._h) == MISMATCH
    assert lib.zk_fri_fold(other._h, layer._h, 1, fp, fp, out1._h) == MISMATCH
    for arity in (0, 4):
        assert lib.zk_fri_fold(ctx._h, layer._h, arity, fp, fp, out1._h) == BAD
    assert lib.zk_fri_fold(ctx._h, layer._h, 1, zp, fp, out1._h) == BAD               # shift = 0
    assert lib.zk_fri_fold(ctx._h, layer._h, 1, pp, fp, out1._h) == BAD               # not fully reduced
    assert lib.zk_fri_fold(ctx._h, layer._h, 1, fp, pp, out1._h) == BAD
    assert lib.zk_fri_fold(ctx._h, layer._h, 1, fp, fp, out3._h) == BAD               # out of the wrong size
    assert lib.zk_fri_fold(ctx._h, layer._h, 3, fp, fp, out1._h) == BAD
    assert lib.zk_fri_fold(ctx._h, layer._h, 1, fp, fp, layer._h) == BAD              # out == in
    assert lib.zk_fri_fold(ctx._h, tiny._h, 2, fp, fp, out1._h) == EVAL_LEN           # fewer variables than the arity
    assert np.array_equal(layer.evaluation_slice(), before)
    assert lib.zk_fri_fold(ctx._h, layer._h, 1, fp, zp, out1._h) == 0                 # beta = 0 is a challenge like any other
    # zk_fri_lde
    assert lib.zk_fri_lde(ctx._h, poly_other._h, 4, fp, c.byref(h)) == MISMATCH
    assert lib.zk_fri_lde(ctx._h, poly._h, 3, fp, c.byref(h)) == BAD                  # 16 coefficients, 8 points
    assert lib.zk_fri_lde(ctx._h, poly._h, 4, zp, c.byref(h)) == BAD
    assert lib.zk_fri_lde(ctx._h, poly._h, 4, pp, c.byref(h)) == BAD
    assert lib.zk_fri_lde(ctx._h, poly._h, 29, fp, c.byref(h)) == NO_ROOT             # BN254: two-adicity 28
    assert not h.value
    # zk_fri_prove
    seed = np.arange(32, dtype=np.uint8)
    sp = seed.ctypes.data_as(u8p)
    buf = np.full(ref.proof_bytes(4, 2, 2, 0, 8), 7, dtype=np.uint8)
    bp = buf.ctypes.data_as(u8p)
    assert lib.zk_fri_prove(other._h, poly._h, 4, 2, 2, 0, 8, fp, sp, bp) == MISMATCH
    for bad in ((4, 2, 0, 0, 8), (4, 2, 4, 0, 8), (4, 0, 2, 0, 8), (4, 9, 2, 0, 8), (4, 2, 2, 0, 0), (4, 2, 2, 0, 1025), (4, 2, 2, 4, 8), (4, 2, 3, 0, 8),
                (3, 2, 1, 0, 8)):   # the last: 16 coefficients against a bound of 8
        assert lib.zk_fri_prove(ctx._h, poly._h, *bad, fp, sp, bp) == BAD, bad
    assert lib.zk_fri_prove(ctx._h, poly._h, 4, 2, 2, 0, 8, zp, sp, bp) == BAD
    assert lib.zk_fri_prove(ctx._h, poly._h, 4, 2, 2, 0, 8, pp, sp, bp) == BAD
    assert lib.zk_fri_prove(ctx._h, poly._h, 27, 2, 3, 0, 8, fp, sp, bp) == NO_ROOT
    assert (buf == 7).all()                                                           # nothing was written by any of them
    assert lib.zk_fri_prove(ctx._h, poly._h, 4, 2, 2, 0, 8, fp, sp, bp) == 0
    assert buf.tobytes() == ref.prove(field, list(range(1, 17)), 4, 2, 2, 0, 8, 5, seed.tobytes())
    # the measurement hook gives a time on every path and leaves the input alone
    for arity, out in ((1, out1), (3, out3)):
        for path in (0, 1, 2):
            ms.value = -1.0
            assert lib.zk_bench_fri_fold(ctx._h, layer._h, arity, out._h, path, 2, c.byref(ms)) == 0 and ms.value > 0, (arity, path)
            assert zk_amd.bench_fri_fold(layer, arity, out, path=path, reps=1) > 0
    ms.value = -1.0
    assert lib.zk_bench_fri_fold(ctx._h, layer._h, 1, out1._h, 3, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_fri_fold(ctx._h, layer._h, 1, out1._h, 0, 0, c.byref(ms)) == BAD
    assert lib.zk_bench_fri_fold(ctx._h, layer_other._h, 1, out1._h, 0, 1, c.byref(ms)) == MISMATCH
    assert lib.zk_bench_fri_fold(ctx._h, layer._h, 1, out3._h, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_fri_fold(ctx._h, tiny._h, 2, out1._h, 0, 1, c.byref(ms)) == EVAL_LEN
    assert ms.value == -1.0 and np.array_equal(layer.evaluation_slice(), before)
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_fri.cpp over zk.hpp: LDE, folds against the LDE of the folded coefficients, proofs, the verifier's verdicts"""
    exe = str(tmp_path / "test_fri")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fri.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: fri host tests passed" in r.stdout
