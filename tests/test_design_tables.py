"""DESIGN.md's measured block is GENERATED from the artefacts under profiles/ (tools/gen_design_tables.py): a number in the
document that differs from the committed bench line / rocprofv3 CSV it cites fails this test (a hand-copied
126.06 us next to a CSV that said 126.63).  Also keeps the document a document: what ships in <= 300 hand-written lines (the generated block not counted), the history elsewhere."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_design_section5_matches_the_artefacts():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_design_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_design_is_a_document_and_history_is_kept():
    lines = open(os.path.join(ROOT, "DESIGN.md")).read().splitlines()
    # the hand-written text is what the limit is about: the generated block's length is the generator's (round 6 added the driver's
    # record beside the builder-box numbers and the batch rows to it)
    a = next(i for i, l in enumerate(lines) if "BEGIN GENERATED" in l)
    z = next(i for i, l in enumerate(lines) if "END GENERATED" in l)
    written = len(lines) - (z - a + 1)
    assert written <= 300, written
    assert os.path.exists(os.path.join(ROOT, "HISTORY.md"))
    text = "\n".join(lines)
    for section in ("## 1. The path and its boundary", "## 4. Kernels", "## 5. Measurement", "## 6. Multi-GPU", "## 7. Oracle and parity",
                    "## 8. Out of scope"):
        assert section in text, section


def test_every_env_switch_of_the_library_is_documented_in_the_header():
    import re

    src = ""
    for d, _, files in os.walk(os.path.join(ROOT, "zk_amd", "csrc")):   # every source file, as tests/test_switch_coverage.py reads them
        for f in sorted(files):
            if f.endswith((".hip", ".cuh", ".hpp", ".inc")):
                src += open(os.path.join(d, f), errors="replace").read()
    names = set(re.findall(r'env_(?:u64|flag)\(\s*"(ZK_[A-Z0-9_]+)"', src))
    assert len(names) > 20, sorted(names)
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    missing = sorted(n for n in names if n not in header)
    assert not missing, missing
