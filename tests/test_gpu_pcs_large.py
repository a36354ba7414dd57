"""The polynomial commitment on the device past the sizes of tests/test_gpu_pcs.py: the first further trip of every loop and second-level
launch on its path (tests/pcs_ref.py names each shape with its arithmetic; tests/test_pcs_large_host.py asserts that arithmetic).

  wide  more than one batch of 32 column pointers (k_pcs_put_ptrs with base > 0): quotients of 32, 33, 64, 65 and 1024 columns and
        openings of width 66, 72 and 1024, the last with 513 queries so that the trace gather has more items than the capped grid has
        threads (k_fri_gather's second sweep) -- byte for byte against the definition
  mid   several partial sums per polynomial in k_pcs_eval_partial / k_pcs_eval_final (d = 13, 14, 15), on every setting of
        ZK_FRI_FUSED_FOLD, and the quotient sizes 1, 2^5 and 2^9 -- byte for byte against the definition
  big   BN254: quotients of 2^20 and 2^21 points (k_pcs_totals with 2 and 4 chunk products per thread) against their half-size
        quotients and sampled outputs, and one opening of two polynomials of 2^19 coefficients (the second trip of the evaluation's
        stride loop, 64 partials) whose values, root and verdicts are computed without the device

Everything is exact field arithmetic: every comparison is equality of bytes or of Python integers."""
import os
import subprocess
import sys

import pytest

import zk_amd
from oracle import binding as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_ref  # noqa: E402
import pcs_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from pcs_large_check import SETTINGS, SWITCH, big_quotient_key, case_key, digest, quotient_key  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "pcs_large_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BIG_QUOTIENT_CHECKS = ("even_odd", "input_intact", "sampled", "half_even_sampled", "half_odd_sampled", "completed")
BIG_OPENING_CHECKS = ("length", "values", "root", "host_verifier_accepts", "definition_accepts", "other_z_rejected", "changed_value_rejected",
                      "flipped_row_byte_rejected", "completed")


@pytest.fixture(scope="module")
def child_lines():
    """{setting: the split lines of the child's output}: one child process per switch setting, side by side (the default child does
    most of the work, much of it on the CPU)"""
    procs = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        procs[setting] = subprocess.Popen([sys.executable, CHECK, setting], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    out, failed = {}, []
    for setting, proc in procs.items():
        try:
            stdout, stderr = proc.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            proc.kill()
            stdout, stderr = proc.communicate()
            failed.append(f"{setting} timed out\n{stdout[-4000:]}\n{stderr[-4000:]}")
            continue
        if proc.returncode != 0 or f"pcs large {setting} ok" not in stdout:
            failed.append(f"{setting} exit {proc.returncode}\n{stdout[-4000:]}\n{stderr[-4000:]}")
        out[setting] = [ln.split() for ln in stdout.splitlines()]
    assert not failed, "\n".join(failed)
    return out


@pytest.fixture(scope="module")
def children(child_lines):
    """{setting: {(kind, field id, key): the rest of the line}}: the digest, and for a proof the host verifier's verdict"""
    return {setting: {(ln[0], ln[1], ln[2]): ln[3:] for ln in lines if ln and ln[0] in ("QUO", "PROOF")} for setting, lines in child_lines.items()}


@pytest.fixture(scope="module")
def big_checks(child_lines):
    """{setting: {(case key, check): the rest of its BIG line}}"""
    return {setting: {(ln[1], ln[2]): ln[3:] for ln in lines if ln and ln[0] == "BIG"} for setting, lines in child_lines.items()}


def _expected_quotients(sizes_of):
    out = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for log_n, k in sizes_of(fi):
            cols = ref.quotient_columns(p, fi, log_n, k, worst_case_values)
            for shift_name, zi, ai in ref.THINNED_COMBOS:
                s, z, alpha, ys = ref.quotient_case(fi, log_n, k, shift_name, zi, ai)
                assert z != s or log_n > 0   # one point: the domain is {s}
                want = ref.quotient(field, cols, s, z, ys, alpha)
                out[("QUO", fri_ref.FIELD_IDS[fi], quotient_key(log_n, k, shift_name, zi, ai))] = digest(orc.from_ints(field, want).tobytes())
    return out


def _expected_proofs(cases, verify):
    """{("PROOF", field id, key): digest of root + values + proof} from the definition, which also accepts those that `verify` names"""
    out = {}
    for fi, case in cases:
        k, d, b, a, f, q = case
        polys, shift, seed, z = ref.case_inputs(fi, case)
        committed = ref.commit(fi, polys, d, b, a, shift)
        root = ref.merkle_ref.root(committed[2])
        ys, proof = ref.prove(fi, polys, d, b, a, f, q, shift, seed, z, committed=committed)
        assert ys == [ref.evaluate(fi, co, z) for co in polys]
        if verify(fi, case):
            assert ref.verify(fi, k, d, b, a, f, q, shift, seed, root, z, ys, proof), (fi, case)   # the same bytes as the device's, below
        out[("PROOF", fri_ref.FIELD_IDS[fi], case_key(case))] = digest(root + orc.from_ints(fi, ys).tobytes() + proof)
    return out


def _compare(got, expected):
    assert set(got) == set(expected)
    wrong = sorted(key for key, want in expected.items() if got[key][0] != want)
    assert not wrong, (wrong[:20], len(wrong))


def test_quotients_past_one_pointer_batch(children):
    """zk_deep_quotient of 32, 33, 64 and 65 columns at 2^3 (!RUN), 2^6 (ALONE) and 2^12 points (three launches, the split table) and of
    1024 columns at 2^6, against pcs_ref.quotient byte for byte: from 33 columns on the pointers arrive in more than one
    k_pcs_put_ptrs launch, and k_pcs_apply's Horner loop reads cols[32..].  Worst-case limb columns, each rotated by its index; four
    combinations of shift, z and alpha per shape; the columns are compared with what was uploaded (in the child)"""
    for fi in range(3):
        sizes = ref.wide_quotient_sizes(fi)
        assert ref.WIDE_QUOTIENT_MAX in sizes and {(12, 33), (12, 65)} <= set(sizes) and len(set(sizes)) == len(sizes)
    assert set(ref.wide_quotient_sizes(0)) == {(n, k) for n in ref.WIDE_QUOTIENT_LOGS for k in ref.WIDE_QUOTIENT_COLUMNS} | {ref.WIDE_QUOTIENT_MAX}
    expected = _expected_quotients(ref.wide_quotient_sizes)
    assert len(expected) == 4 * sum(len(ref.wide_quotient_sizes(fi)) for fi in range(3))
    wide = {k for fi in range(3) for _, k in ref.wide_quotient_sizes(fi)}
    _compare({key: rest for key, rest in children["default"].items() if key[0] == "QUO" and int(key[2].split("_")[1][1:]) in wide}, expected)


def test_quotient_sizes_between_the_tested_ones(children):
    """zk_deep_quotient at N = 1 (log_n = 0: no table bits, w = 1; z differs from s, the one point of the domain), 2^5 (the largest
    launch without wave runs) and 2^9 (one workgroup whose rows q >= 2 lie wholly outside) over 1, 2 and 3 columns, byte for byte"""
    expected = _expected_quotients(ref.edge_quotient_sizes)
    assert len(expected) == 3 * 4 * len(ref.EDGE_QUOTIENT_LOGS) * len(ref.EDGE_QUOTIENT_COLUMNS)
    edge = set(ref.EDGE_QUOTIENT_COLUMNS)
    _compare({key: rest for key, rest in children["default"].items() if key[0] == "QUO" and int(key[2].split("_")[1][1:]) in edge}, expected)
    assert not any(key[0] == "QUO" for setting in ("fused", "binary") for key in children[setting])   # no switch reaches the quotient


def test_openings_past_one_pointer_batch_and_one_gather_sweep(children):
    """root, values and proof of zk_pcs_commit / zk_pcs_open against pcs_ref.prove, byte for byte, at widths 66, 72 and -- on every
    field -- 1024 = kPcsMaxColumns = kMerkleMaxColumns with 513 queries: 525,825 gather items on 524,288 threads, so the rows and
    paths of the last queries come from k_fri_gather's second sweep.  zk_pcs_verify_host accepted each (in the child); pcs_ref.verify
    accepts the same bytes (the 17 MB proofs on one field)"""
    assert ref.gather_items(ref.WIDE_MAX_CASE) > ref.GATHER_THREADS and ref.WIDE_MAX_CASE[0] << ref.WIDE_MAX_CASE[3] == ref.MAX_COLUMNS
    assert {fi for fi, case in ref.WIDE_CASES if case == ref.WIDE_MAX_CASE} == {0, 1, 2}
    expected = _expected_proofs(ref.WIDE_CASES, lambda fi, case: case != ref.WIDE_MAX_CASE or fi == ref.WIDE_VERIFY_FIELD)
    mid = {("PROOF", fri_ref.FIELD_IDS[fi], case_key(case)) for fi, case in ref.MID_CASES}
    got = {key: rest for key, rest in children["default"].items() if key[0] == "PROOF" and key not in mid}
    _compare(got, expected)
    assert all(rest[1] == "accepted" for rest in got.values()), got


@pytest.fixture(scope="module")
def expected_mid():
    return _expected_proofs(ref.MID_CASES, lambda fi, case: True)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_openings_with_several_partials_per_polynomial(children, expected_mid, setting):
    """d = 13, 14, 15: k_pcs_eval_partial on 2, 4 and 8 workgroups per polynomial (its blockIdx.y gridDim.x + blockIdx.x indexing, z^j0
    for j0 >= 4096) and k_pcs_eval_final adding several partials; polynomials of 2^d, 2^d - 1 and fewer coefficients; root, values and
    proof byte for byte against pcs_ref.prove with the fused fold kernel, with the binary launches and by default"""
    assert [ref.eval_partials(case[1]) for _, case in ref.MID_CASES] == [2, 4, 8]
    got = {key: rest for key, rest in children[setting].items() if key in expected_mid}
    _compare(got, expected_mid)
    assert all(rest[1] == "accepted" for rest in got.values()), got
    if setting != "default":   # these children run nothing else
        assert set(children[setting]) == set(expected_mid)


def _all_pass(checks, key, names):
    assert {name for case, name in checks if case == key} == set(names)
    failed = sorted((name, rest) for (case, name), rest in checks.items() if case == key and rest[0] != "PASS")
    assert not failed, (key, failed)


@pytest.mark.parametrize("log_n,k", ref.BIG_QUOTIENTS)
def test_quotients_with_several_chunk_products_per_thread(big_checks, log_n, k):
    """zk_deep_quotient at 2^20 points over 3 columns and 2^21 over 1, BN254, seeded columns, s, z, alpha and values: 512 and 1024 chunk
    products on the 256 threads of k_pcs_totals, whose prefix and back-substitution loops over inv[] take 2 and 4 trips.  On the
    device, the whole output against the interleaved quotients of the even rows (shift s) and of the odd rows (shift s w_N), which
    have half as many chunks (2^19 points: one per thread, every thread busy); 4096 outputs (the ends, the first run, chunk and table
    split, both sides of the threads' run boundaries, seeded ones) against pcs_ref.quotient_at on the downloaded columns, 256 of each
    half the same way; the columns left intact"""
    assert ref.totals_per_thread(log_n) == {20: 2, 21: 4}[log_n] and ref.totals_per_thread(log_n - 1) == {20: 1, 21: 2}[log_n]
    _all_pass(big_checks["default"], big_quotient_key(log_n, k), BIG_QUOTIENT_CHECKS)


def test_opening_of_two_polynomials_of_2_19_coefficients(big_checks):
    """(k, d, b, a, f, Q) = (2, 19, 1, 3, 1, 8), BN254, 2^19 and 2^19 - 1 seeded coefficients: 32,768 runs of 16 coefficients per
    polynomial on 64 x 256 threads, so k_pcs_eval_partial's loop takes two trips and k_pcs_eval_final adds 64 partials; the quotient
    of 2^20 points goes through k_pcs_totals with two chunk products per thread and k_pcs_apply's TIMES_X form.  The values against Horner over
    Python integers; the root against merkle_ref.commit_bulk over the LDEs by the oracle's transform (nothing downloaded);
    zk_pcs_verify_host and pcs_ref.verify (under that root) accept, and reject another z, a changed value and a flipped byte in a
    commitment row.  Acceptance pins the queried positions only: the big quotients above pin the rest of that kernel"""
    assert ref.eval_partials(ref.BIG_CASE[1]) == 64 and (1 << ref.BIG_CASE[1]) // ref.EVAL_RUN > ref.EVAL_MAX_BLOCKS * ref.EVAL_THREADS
    _all_pass(big_checks["default"], case_key(ref.BIG_CASE), BIG_OPENING_CHECKS)
    assert not big_checks["fused"] and not big_checks["binary"]
