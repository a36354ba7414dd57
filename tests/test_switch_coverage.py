"""zk_amd/csrc/env.hpp says the tests force every kernel-selecting ZK_* switch in a child process.  This keeps it true: every switch
name read with env_u64 / env_flag anywhere under zk_amd/csrc must be named in some file under tests/, except the debug and timing
switches listed here, which select no kernel."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXEMPT = {"ZK_BATCH_DEBUG", "ZK_HOST_DEBUG", "ZK_PIPE_DEBUG", "ZK_SHARD_FAKE_ALLREDUCE_US"}


def _read_tree(top, suffixes, skip=()):
    out = {}
    for d, _, files in os.walk(top):
        for f in files:
            if f.endswith(suffixes) and f not in skip:
                out[os.path.join(d, f)] = open(os.path.join(d, f), errors="replace").read()
    return out


def test_every_kernel_selecting_switch_is_named_by_a_test():
    src = "\n".join(_read_tree(os.path.join(ROOT, "zk_amd", "csrc"), (".hip", ".cuh", ".hpp", ".inc")).values())
    names = set(re.findall(r'env_(?:u64|flag)\(\s*"(ZK_[A-Z0-9_]+)"', src))
    assert len(names) > 20 and EXEMPT <= names, sorted(EXEMPT - names)
    tests = "\n".join(_read_tree(os.path.join(ROOT, "tests"), (".py", ".cpp", ".hip", ".hpp"), skip=(os.path.basename(__file__),)).values())
    unnamed = sorted(n for n in names - EXEMPT if not re.search(r"\b%s\b" % n, tests))
    assert not unnamed, f"switches that no test names (force them in a child process, or list a debug switch in EXEMPT): {unnamed}"
