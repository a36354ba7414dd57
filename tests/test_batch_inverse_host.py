"""The definition of batch inversion and running products (tests/batch_inverse_ref.py) checked on its own, the shared case
generators, the kernel's chunk size against the source, and the new exports' argument checks -- all without a GPU."""
import ctypes as c
import os
import re
import sys

import numpy as np

from oracle import binding as orc
from zk_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_inverse_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -20


def test_definition_by_brute_force_mod_17():
    p = 17
    for shift in range(p):
        out, zeros = ref.batch_inverse(list(range(p)), shift, p)
        assert zeros == 1
        for v, inv in zip(range(p), out):
            x = (v + shift) % p
            assert (inv == 0) if x == 0 else (x * inv % p == 1 and 0 < inv < p)
            assert inv == ([y for y in range(p) if x * y % p == 1] or [0])[0]   # the only inverse there is
    assert ref.batch_inverse([], 3, p) == ([], 0)
    assert ref.batch_inverse([0, 0, 5], 0, p) == ([0, 0, 7], 2)
    assert ref.prefix_product([2, 3, 4], False, p) == ([1, 2, 6], 24 % p)
    assert ref.prefix_product([2, 3, 4], True, p) == ([2, 6, 24 % p], 24 % p)
    assert ref.prefix_product([2, 0, 4], True, p) == ([2, 0, 0], 0)   # a zero propagates
    assert ref.prefix_product([2, 0, 4], False, p) == ([1, 2, 0], 0)
    assert ref.prefix_product([], False, p) == ([], 1)


def test_definition_on_the_real_moduli():
    for field in range(3):
        p = orc.modulus(field)
        _, r1, _, _ = orc.field_constants(field)
        vals = [1, 2, p - 1, r1]
        out, zeros = ref.batch_inverse(vals, 0, p)
        assert zeros == 0 and out[0] == 1 and out[1] == (p + 1) // 2 and out[2] == p - 1
        assert all(v * i % p == 1 for v, i in zip(vals, out))
        # the C oracle's own inversion agrees (Montgomery limbs in and out)
        for v, i in zip(vals, out):
            assert orc.to_int(field, orc.inverse(field, orc.from_int(field, v))) == i
        cache = {}
        assert ref.batch_inverse(vals, 5, p, cache) == ref.batch_inverse(vals, 5, p) == ref.batch_inverse(vals, 5, p, cache)
        assert ref.batch_inverse([p - 5, 1], 5, p) == ([0, pow(6, p - 2, p)], 1)


def test_generators_produce_the_zero_placements():
    C, B, E = ref.CHUNK, ref.BLOCK, ref.PER_THREAD
    z = ref.zero_placements(2 * C + 1)
    assert z["zero_at_0"] == [0] and z["zero_at_last"] == [2 * C]
    assert z["group_first_and_last"] == [5, (E - 1) * B + 5]                       # the last chunk holds one element: nothing of thread 5
    assert z["chunk_first_and_last"] == [0, C - 1, C, 2 * C - 1, 2 * C]
    assert z["whole_chunk"] == [2 * C] and z["all_zero"] == list(range(2 * C + 1))
    assert z["two_adjacent"] == [C, C + 1]
    z = ref.zero_placements(C + 1 + B)
    assert z["whole_group"] == [C + 5] and z["whole_chunk"] == list(range(C, C + 1 + B))
    z = ref.zero_placements(C)
    assert z["whole_group"] == [q * B + 5 for q in range(E)]                        # every element of thread 5
    assert z["group_first_and_last"] == [5, (E - 1) * B + 5]
    assert z["whole_chunk"] == list(range(C)) and z["chunk_first_and_last"] == [0, C - 1]
    assert all(v == [] for v in ref.zero_placements(0).values())
    assert ref.zero_placements(1)["two_adjacent"] == [0] and ref.zero_placements(2)["two_adjacent"] == [1]
    assert ref.LENGTHS == (0, 1, 2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1)
    assert ref.MLE_VARS == (0, 1, 6, ref.LOG_CHUNK - 1, ref.LOG_CHUNK, ref.LOG_CHUNK + 1) and 1 << ref.LOG_CHUNK == C
    p = orc.modulus(0)
    names = ["random", "random_shift", "zero_at_0", "zero_at_last", "group_first_and_last", "chunk_first_and_last", "whole_group",
             "whole_chunk", "all_zero", "two_adjacent", "zero_by_shift_only"]
    for n in (0, 1, 65, C + 1):
        cs = ref.cases(p, 0, n, worst_case_values)
        assert [name for name, _, _ in cs] == names
        by = {name: (v, s) for name, v, s in cs}
        assert all(len(v) == n and all(0 <= x < p for x in v) for v, _ in by.values())
        assert 0 not in by["random"][0] and by["random"][1] == 0 and by["random_shift"][1] != 0
        for name, idx in ref.zero_placements(n).items():
            assert [i for i, x in enumerate(by[name][0]) if x == 0] == idx
        v, s = by["zero_by_shift_only"]
        assert 0 not in v and ref.batch_inverse(v, s, p)[1] == len(set(ref.zero_placements(n)["chunk_first_and_last"] + ref.zero_placements(n)["two_adjacent"]))
    big = ref.base_values(p, 0, 300, worst_case_values)
    assert p - 1 in big and 1 in big   # the worst-case limbs are in


def test_chunk_constants_match_the_kernel_source():
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "inv_kernels.cuh")).read()
    common = open(os.path.join(ROOT, "zk_amd", "csrc", "common.cuh")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    per = int(re.search(r"constexpr uint32_t kInvPerThread = (\d+);", src).group(1))
    assert re.search(r"constexpr uint32_t kInvChunk = kBlock \* kInvPerThread;", src)
    assert (ref.BLOCK, ref.PER_THREAD, ref.CHUNK) == (block, per, block * per)
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    assert re.search(r"ZK_BATCH_INV_ONE_LAUNCH_MAX\s+%d\s+0 \.\. %d\b" % (ref.CHUNK, ref.CHUNK), header)   # the switch's default and range


def test_new_exports_reject_null_arguments_without_gpu():
    lib = _lib.lib
    buf = np.zeros(4, dtype=np.uint64)
    bp = buf.ctypes.data_as(_lib.u64p)
    h = c.c_void_p()
    ms = c.c_double()
    fake = c.c_void_p(8)   # never dereferenced: a NULL among the others ends the call first
    assert lib.zk_mle_batch_inverse(None, fake, None, fake, None) == BAD
    assert lib.zk_mle_batch_inverse(fake, None, None, fake, None) == BAD
    assert lib.zk_mle_batch_inverse(fake, fake, None, None, None) == BAD
    assert lib.zk_upoly_batch_inverse(None, fake, None, c.byref(h), None) == BAD
    assert lib.zk_upoly_batch_inverse(fake, None, None, c.byref(h), None) == BAD
    assert lib.zk_upoly_batch_inverse(fake, fake, None, None, None) == BAD
    assert h.value is None
    assert lib.zk_mle_prefix_product(None, fake, 0, fake, None) == BAD
    assert lib.zk_mle_prefix_product(fake, None, 1, fake, bp) == BAD
    assert lib.zk_mle_prefix_product(fake, fake, 0, None, None) == BAD
    assert lib.zk_batch_inverse_host(None, bp, 1, None, bp, None) == BAD
    assert lib.zk_batch_inverse_host(fake, None, 1, None, bp, None) == BAD
    assert lib.zk_batch_inverse_host(fake, bp, 1, None, None, None) == BAD
    assert lib.zk_bench_batch_inverse(None, fake, fake, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_batch_inverse(fake, None, fake, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_batch_inverse(fake, fake, None, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_batch_inverse(fake, fake, fake, 0, 1, None) == BAD
    assert lib.zk_bench_batch_inverse(fake, fake, fake, 0, 0, c.byref(ms)) == BAD    # reps < 1
    assert lib.zk_bench_batch_inverse(fake, fake, fake, 4, 1, c.byref(ms)) == BAD    # no such path
    assert lib.zk_bench_batch_inverse(fake, fake, fake, -1, 1, c.byref(ms)) == BAD
    assert not buf.any()


def test_binary_inverse_equals_the_fermat_inverse_on_the_host(tmp_path):
    """zk_amd/csrc/inv_field.cuh compiled for the CPU (tests/cpp/test_inverse_host.cpp): the one inversion a batch call makes, against
    the host's Fermat inverse on random and edge values of all three fields"""
    import shutil
    import subprocess

    cxx = "/opt/rocm/lib/llvm/bin/clang++"   # field.cuh uses __builtin_addc: clang, as tests/cpp/Makefile builds test_field_host
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    assert cxx, "no clang++ to build the host harness with"
    exe = str(tmp_path / "test_inverse_host")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_inverse_host.cpp")],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: binary inverse equals the Fermat inverse" in r.stdout
