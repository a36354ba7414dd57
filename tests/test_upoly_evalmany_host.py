"""zk_upoly_evaluate_many without a GPU: the Python restatement of the transposed subproduct tree (tests/evalmany_ref.py, the steps
the device's tree path runs) against Horner in the three fields, the new symbols in the header, the ctypes table, the C++ mirror
and the Rust shim, and argument checks that answer before any device work."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from zk_amd import _lib
from zk_amd._lib import ZkError, c, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evalmany_ref import evaluate_many_tree, horner, horner_many, invert_series, up_sweep  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zk_upoly_evaluate_many", "zk_upoly_evaluate_many_host", "zk_bench_upoly_evaluate_many"]
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]


def _no_gpu():
    import torch

    return not torch.cuda.is_available()


@pytest.mark.parametrize("field", FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
@pytest.mark.parametrize("stop", [1, 4, 8])
def test_transposed_tree_restatement_matches_horner(field, stop):
    """N = 8 .. 64, the recursion stopped at nodes of `stop` points (the device stops at 2^7), L != n, repeated and zero points"""
    p = zk_amd.modulus(field)
    rng = random.Random(1000 * field + stop)
    shapes = [(8, 8), (16, 16), (32, 32), (64, 64), (5, 13), (13, 5), (33, 20), (7, 64), (64, 9), (1, 8), (0, 9), (24, 24)]
    for L, n in shapes:
        co = [rng.randrange(p) for _ in range(L)]
        xs = [rng.randrange(p) for _ in range(n)]
        xs[1], xs[2], xs[n - 1] = xs[0], 0, p - 1
        assert evaluate_many_tree(co, xs, p, stop) == horner_many(co, xs, p), (L, n)
    assert evaluate_many_tree([3, 4], [5] * 8, p, stop) == [23] * 8            # one point eight times
    assert evaluate_many_tree([0] * 8, list(range(8)), p, stop) == [0] * 8     # the zero polynomial
    assert evaluate_many_tree([1, 2, 3], [], p, stop) == []


def test_restatement_pieces():
    p = (1 << 61) - 1
    xs = [3, 5, 7, 11]
    lv = up_sweep(xs, p)
    # (x - 3)(x - 5)(x - 7)(x - 11) = x^4 - 26x^3 + 236x^2 - 886x + 1155
    assert lv[2] == [1155, (-886) % p, 236, (-26) % p]
    assert lv[1] == [15, p - 8, 77, p - 18]
    R = [1] + [lv[2][4 - k] for k in range(1, 4)]
    alpha = invert_series(R, 4, p)
    prod = [sum(R[i] * alpha[k - i] for i in range(k + 1)) % p for k in range(4)]
    assert prod == [1, 0, 0, 0]
    assert horner([1, 2, 3], 2, p) == 17 and horner([], 5, p) == 0


def test_evalmany_symbols_are_declared_exported_and_typed():
    declared = _lib.declared_symbols()
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    mirror = open(os.path.join(ROOT, "zk_amd", "host", "zk.hpp")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in _lib._sig, n
        assert getattr(lib, n).restype is c.c_int32
        assert re.search(r"int32_t %s\(zk_ctx \*ctx," % n, header), n
    assert lib.zk_abi_version() == 6   # symbols only
    assert "zk_upoly_evaluate_many(context<F>()" in mirror and "UnivariatePolynomial evaluate_many(const UnivariatePolynomial &xs) const" in mirror
    assert "fn zk_upoly_evaluate_many(ctx: *mut zk_ctx, p: *const zk_upoly, xs: *const zk_upoly, out: *mut *mut zk_upoly) -> i32;" in shim
    impl = shim[shim.index("impl<F: GpuField> UnivariatePolynomial<F> {"):]
    assert re.search(r"pub fn evaluate_many\(&self, xs: &Self\) -> Result<Self, &'static str> \{", impl)
    assert hasattr(zk_amd.UnivariatePolynomial, "evaluate_many") and hasattr(zk_amd, "upoly_evaluate_many_host")
    # both switches are documented where the others are
    for switch in ("ZK_UPOLY_EVALMANY_DIRECT_MAX", "ZK_UPOLY_INTERP_XY_TREE_MIN"):
        assert switch in header and switch in open(os.path.join(ROOT, "INTEGRATION.md")).read(), switch


def test_evalmany_argument_checks_need_no_device():
    h = c.c_void_p()
    assert lib.zk_upoly_evaluate_many(None, None, None, c.byref(h)) == -20
    assert lib.zk_upoly_evaluate_many_host(None, None, 0, None, 0, None) == -20
    assert lib.zk_bench_upoly_evaluate_many(None, None, None, 0, 1, None) == -20


def test_evalmany_without_gpu_fails_loudly():
    if not _no_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ZkError) as e:
        zk_amd.upoly_evaluate_many_host(zk_amd.Context(zk_amd.BN254_FR, 0), np.zeros((3, 4), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64))
    assert e.value.code == -22   # ZK_ERR_NO_DEVICE


def test_cpp_evalmany_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_upoly_evalmany")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_upoly_evalmany.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    if not _no_gpu():
        pytest.skip("GPU present: run by tests/test_gpu_upoly_evalmany.py")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr
