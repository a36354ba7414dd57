"""The field primitives ON THE DEVICE, one operation at a time: tests/cpp/test_field_device.hip runs every primitive of field.cuh
and the [0, 2p) helpers of ntt_kernels.cuh over the corpus of tests/field_corpus.py, as shipped (the v_mad_u64_u32 / v_addc_co_u32
chains) and built with -DZK_NO_ASM, and every output limb is compared with Python integers.  The harness runs once per field and
build in a child process under its own time limit; a child that fails is reported with what it left behind and nothing runs after
it."""
import os
import subprocess
import time

import pytest

import field_corpus as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BUILDS = {"asm": "test_field_device", "no_asm": "test_field_device_noasm"}
CHILD_TIMEOUT = 180   # seconds: ten million cases are well under a second of kernels; the rest is process start and 400 MB of file I/O


@pytest.mark.gpu
def test_field_primitives_on_device_match_big_int_model(tmp_path):
    r = subprocess.run(["make", "-C", CPP, "test_field_device", "test_field_device_noasm"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    t0 = time.time()
    tasks = []
    for field in range(3):
        fm, secs = fc.built(field)
        cases = str(tmp_path / f"cases_{field}.bin")
        with open(cases, "wb") as f:
            f.write(fc.case_file_bytes(field, secs))
        outputs = {}
        for build, binary in BUILDS.items():
            out = str(tmp_path / f"out_{field}_{build}.bin")
            try:
                r = subprocess.run([os.path.join(CPP, binary), cases, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
                rc, log = r.returncode, r.stdout + r.stderr
            except subprocess.TimeoutExpired as e:
                rc, log = "timeout", f"{e.stdout or ''}{e.stderr or ''}"
            # no retry and nothing else on the GPU after a failed child
            assert rc == 0, (f"{binary} on {fc.FIELD_NAMES[field]}: exit {rc}; output file "
                             f"{'has %d bytes' % os.path.getsize(out) if os.path.exists(out) else 'missing'}; log:\n{log[-4000:]}")
            outputs[build] = out
        tasks += [(field, i, outputs, ()) for i in range(len(secs))]
    t_gpu = time.time() - t0
    results = fc.run_checks(tasks)
    n_cases = sum(r["n"] for r in results)
    print(f"\n{'primitive':20s} " + " ".join(f"{fc.FIELD_NAMES[f] + ' ' + b:>18s}" for f in range(3) for b in BUILDS) + "   (mismatching limbs)")
    failures = []
    for op in range(len(fc.OP_NAMES)):
        row = []
        for field in range(3):
            for build in BUILDS:
                rs = [r for r in results if r["op"] == op and r["field"] == field]
                row.append(sum(abs(r["builds"][build]["bad_limbs"]) for r in rs))
        print(f"{fc.OP_NAMES[op]:20s} " + " ".join(f"{v:18d}" for v in row))
    for r in results:
        b = r["builds"]
        if b["asm"]["bad_limbs"] or b["no_asm"]["bad_limbs"]:
            bad = "asm" if b["asm"]["bad_limbs"] else "no_asm"
            first = b[bad]["first"] or {"note": b[bad].get("note")}
            if b["asm"]["bad_limbs"] and not b["no_asm"]["bad_limbs"]:
                verdict = "the ZK_NO_ASM build agrees with the model: the asm chain is at fault"
            elif b["asm"]["bad_limbs"]:
                verdict = "the ZK_NO_ASM build disagrees with the model too: the algorithm is at fault"
            else:
                verdict = "only the ZK_NO_ASM build disagrees with the model: the plain C++ body is at fault"
            failures.append(f"{fc.OP_NAMES[r['op']]} on {fc.FIELD_NAMES[r['field']]} [{r['label']}]: {b[bad]['bad_limbs']} limbs differ in the "
                            f"{bad} build; first failing case {first}; {verdict}")
    print(f"{n_cases} cases x {len(BUILDS)} builds; harness runs {t_gpu:.1f} s, whole test {time.time() - t0:.1f} s")
    assert not failures, "\n".join(failures[:10])
    assert n_cases > 30_000_000
