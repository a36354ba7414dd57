"""Conditions that keep the field-primitive corpus (tests/field_corpus.py) from being toothless, checked with the big-int model
alone, and the model itself checked against the host compilation of field.cuh before a GPU sees it.  No GPU needed."""
import os
import subprocess

import pytest

import field_corpus as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
MIN_SIDE = 256   # cases on each side of every final conditional step, per primitive and field

# primitive -> the conditional step its cases exercise
BRANCHES = {
    fc.OP_ADD: "fe_add: sub8 of s >= p",
    fc.OP_SUB: "fe_sub: borrow, add p back",
    fc.OP_MUL: "redc: sub8 of s >= p (fe_mul)",
    fc.OP_MULWIDE_REDC: "redc: sub8 of s >= p (mul_wide + redc)",
    fc.OP_FROM_CANONICAL: "redc: sub8 of s >= p (fe_from_canonical)",
    fc.OP_MUL29: "mul29_core: sub8 of s >= p (fe_mul29)",
    fc.OP_MUL_TT: "mul29_core: sub8 of s >= p (fe_mul_tt)",
    fc.OP_DOT2: "mul29_core<TWO>: sub8 of s >= p (fe_dot2_29)",
    fc.OP_CANON2: "fe_canon2: sub8 of a >= p",
    fc.OP_ADD2: "fe_add2: carry or no borrow, subtract 2p",
    fc.OP_SUB2: "fe_sub2: borrow, add 2p back",
}


@pytest.fixture(scope="module")
def harness():
    """both gfx950 builds of the harness and the host build (make is a no-op when they are current)"""
    r = subprocess.run(["make", "-C", CPP, "field_harness"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return {n: os.path.join(CPP, n) for n in ("test_field_device", "test_field_device_noasm", "test_field_device_host")}


@pytest.fixture(scope="module")
def checked(harness, tmp_path_factory):
    """every section of every field through the model; the sections of field.cuh's own primitives also through the host build of the
    harness (the [0, 2p) helpers of ntt_kernels.cuh are device code: they are modelled here and run on the GPU only)"""
    tmp = tmp_path_factory.mktemp("field_corpus")
    tasks = []
    for field in range(3):
        fm, secs = fc.built(field)
        host_secs = [s for s in secs if s.op not in fc.DEVICE_ONLY]
        cases, out = str(tmp / f"cases_{field}.bin"), str(tmp / f"out_{field}.bin")
        with open(cases, "wb") as f:
            f.write(fc.case_file_bytes(field, host_secs))
        r = subprocess.run([harness["test_field_device_host"], cases, out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        tasks += [(field, i, {"host": out}, fc.DEVICE_ONLY) for i in range(len(secs))]
    return fc.run_checks(tasks)


def test_harness_builds_for_gfx950(harness):
    """as shipped and with -DZK_NO_ASM: two gfx950 code objects from one source; the shipped one carries the asm chains"""
    for name in ("test_field_device", "test_field_device_noasm"):
        assert os.path.exists(harness[name])
        blob = open(harness[name], "rb").read()
        assert b"gfx950" in blob, name


def test_model_matches_host_build_of_field_cuh(checked):
    bad = [(fc.FIELD_NAMES[r["field"]], fc.OP_NAMES[r["op"]], r["label"], r["builds"]["host"]) for r in checked
           if "host" in r["builds"] and r["builds"]["host"]["bad_limbs"] != 0]
    n = sum(r["n"] for r in checked if "host" in r["builds"])
    print(f"model vs host build of field.cuh: {n} cases, {len(bad)} sections with mismatches")
    assert not bad, bad[:3]
    assert n > 3_000_000


def test_each_side_of_every_final_conditional_step_has_cases(checked):
    print(f"\n{'conditional step':58s} {'field':10s} {'taken':>9s} {'not taken':>10s}")
    short = []
    for op, what in BRANCHES.items():
        for field in range(3):
            rs = [r for r in checked if r["op"] == op and r["field"] == field]
            taken = sum(r["taken"] for r in rs)
            not_taken = sum(r["n"] for r in rs) - taken
            print(f"{what:58s} {fc.FIELD_NAMES[field]:10s} {taken:9d} {not_taken:10d}")
            if min(taken, not_taken) < MIN_SIDE:
                short.append((what, fc.FIELD_NAMES[field], taken, not_taken))
    assert not short, short


def test_taken_side_of_fe_mul29_with_canonical_a_is_filtered_in(checked):
    """random canonical pairs take mul29_core's final subtraction in well under 1 % of cases: the corpus searches for them"""
    for field in range(3):
        rs = [r for r in checked if r["field"] == field and r["op"] in (fc.OP_MUL29, fc.OP_MUL29_LAZY) and r["label"].startswith("canonical a")]
        assert len(rs) == 2
        for r in rs:
            assert r["n"] >= MIN_SIDE and (r["taken"] is None or r["taken"] == r["n"]), r


def test_exact_boundaries_are_present(checked):
    def facts(field, op):
        out = set()
        for r in checked:
            if r["field"] == field and r["op"] == op:
                out |= set(r["facts"])
        return out

    for field in range(3):
        name = fc.FIELD_NAMES[field]
        # pre-subtraction value == p (a = p, the lazy-domain zero), p - 1 and p + 1 in the 29-bit core; a + b = p / 2p in the adds
        for op in (fc.OP_MUL29, fc.OP_MUL29_LAZY, fc.OP_ADD, fc.OP_ADD2, fc.OP_CANON2):
            assert {"pre == edge - 1", "pre == edge", "pre == edge + 1"} <= facts(field, op), (name, fc.OP_NAMES[op], facts(field, op))
        # redc and fe_mul_tt multiply values below p: p | a b is impossible, so `== p` cannot occur; its two neighbours must
        for op in (fc.OP_MUL, fc.OP_MULWIDE_REDC, fc.OP_MUL_TT):
            assert {"pre == edge - 1", "pre == edge + 1"} <= facts(field, op), (name, fc.OP_NAMES[op], facts(field, op))
        for op in (fc.OP_ADD, fc.OP_SUB, fc.OP_MUL, fc.OP_MULWIDE_REDC, fc.OP_MUL29, fc.OP_MUL_TT, fc.OP_DOT2):
            assert {"result 0", "result 1", "result p - 1"} <= facts(field, op), (name, fc.OP_NAMES[op], facts(field, op))
        # fe_add2's carry out of 2^256: only where 4p > 2^256
        assert ("carry out of 2^256" in facts(field, fc.OP_ADD2)) == (field == 1), name
        # redc_wide's top limb reaches the field's maximum floor(32 p^2 / 2^512)
        fm = fc.FieldModel(field)
        assert fm.top_max == (1, 6, 0)[field]
        assert f"top limb max {fm.top_max}" in facts(field, fc.OP_WIDE), (name, facts(field, fc.OP_WIDE))


def test_corpus_is_deterministic_and_inside_its_domains():
    for field in range(3):
        fm, secs = fc.build_sections(field)
        assert fc.case_file_bytes(field, secs) == fc.case_file_bytes(field, fc.built(field)[1])
        p = fm.p
        left = {fc.OP_MUL29: fc.R, fc.OP_MUL29_LAZY: fc.R, fc.OP_REDUCE_U256: fc.R, fc.OP_ADD2: 2 * p, fc.OP_SUB2: 2 * p, fc.OP_CANON2: 2 * p,
                fc.OP_FROM_U32: 1 << 32}
        for s in secs:
            cols = [s.cross[0], s.cross[1]] if s.cross else s.cols()
            for j, col in enumerate(cols):
                bound = left.get(s.op, p) if (j == 0 or s.op in (fc.OP_ADD2, fc.OP_SUB2)) else p
                assert all(0 <= v < bound for v in col), (fc.OP_NAMES[s.op], s.label, j)
            if s.op == fc.OP_WIDE:
                assert 1 <= s.param <= fc.K_MAX_LAZY and len(cols) == 2 * s.param
