"""zk_upoly_divrem / zk_upoly_inverse_series without a GPU: the Python restatement of what the device runs (tests/divrem_ref.py: the
Newton inversion, the reversed quotient with the truncated remainder product, the linear divisor's chunked affine scan) against
big-int schoolbook division in the three fields, the new symbols in the header, the ctypes table, the C++ mirror and the Rust shim,
and the argument checks that answer before any device work."""
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
from divrem_ref import (ZeroLead, divrem, divrem_linear_scan, divrem_newton, inverse_series, inverse_series_newton,  # noqa: E402
                        mul)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zk_upoly_divrem", "zk_upoly_inverse_series", "zk_upoly_divrem_host", "zk_upoly_inverse_series_host", "zk_bench_upoly_divrem"]
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BAD, UNSUP = -20, -25


def _no_gpu():
    import torch

    return not torch.cuda.is_available()


def _operands(rng, p, la, lb, variant):
    a = [rng.randrange(p) for _ in range(la)]
    b = [rng.randrange(p) for _ in range(lb - 1)] + [rng.randrange(1, p)]
    if variant == 1 and la >= 3:
        a[-2:] = [0, 0]        # a zero-topped dividend: the zeros stay in q
    if variant == 2 and lb >= 2:
        b[0] = 0
    return a, b


@pytest.mark.parametrize("field", FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def test_newton_restatement_matches_schoolbook(field):
    """la = 0 .. 23, lb = 1 .. 9: la < lb, lb = 1, k = 1, zero-topped a and b[0] = 0 included; a = q b + r holds exactly"""
    p = zk_amd.modulus(field)
    rng = random.Random(2000 + field)
    for la in range(24):
        for lb in range(1, 10):
            a, b = _operands(rng, p, la, lb, (la + lb) % 3)
            q, r = divrem(a, b, p)
            assert len(q) == max(la - lb + 1, 0) and len(r) == (lb - 1 if la >= lb else la)
            assert divrem_newton(a, b, p) == (q, r), (la, lb)
            back = mul(q, b, p) + [0] * la
            assert [(back[i] + (r[i] if i < len(r) else 0)) % p for i in range(la)] == a, (la, lb)
    with pytest.raises(ZeroLead):
        divrem([1, 2, 3], [1, 0], p)
    with pytest.raises(ZeroLead):
        divrem_newton([1, 2, 3], [1, 0], p)
    with pytest.raises(ValueError):
        divrem([1, 2, 3], [], p)
    assert divrem([1, 2], [5, 6, 0], p) == ([], [1, 2])   # la < lb: nothing is inverted


@pytest.mark.parametrize("field", FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def test_affine_scan_with_a_short_top_chunk_matches_schoolbook(field):
    """lb = 2 in chunks of 8 (lane runs of 2) and 16 (runs of 4): whole chunks, a ragged top chunk, one short chunk; z = 1, z = 0"""
    p = zk_amd.modulus(field)
    rng = random.Random(3000 + field)
    for la in (2, 3, 7, 8, 9, 16, 17, 23, 24, 25, 40, 41):
        for b in ([rng.randrange(1, p), rng.randrange(2, p)], [p - 1, 1], [0, 1], [0, rng.randrange(2, p)]):
            a = [rng.randrange(p) for _ in range(la)]
            want = divrem(a, b, p)
            for chunk, run in ((8, 2), (16, 4), (4, 1)):
                assert divrem_linear_scan(a, b, p, chunk, run) == want, (la, b, chunk)
    with pytest.raises(ZeroLead):
        divrem_linear_scan([1, 2, 3], [4, 0], p)


@pytest.mark.parametrize("field", FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def test_inverse_series_times_f_is_one(field):
    p = zk_amd.modulus(field)
    rng = random.Random(4000 + field)
    for k in (0, 1, 2, 3, 5, 6, 7, 11, 16, 17, 31):
        for lf in (1, 2, 5, 40):
            f = [rng.randrange(1, p)] + [rng.randrange(p) for _ in range(lf - 1)]
            g = inverse_series_newton(f, k, p)
            assert g == inverse_series(f, k, p) and len(g) == k
            if k:
                assert mul(f, g, p)[:k] == [1] + [0] * (k - 1), (k, lf)
    with pytest.raises(ZeroLead):
        inverse_series([0, 1], 3, p)
    with pytest.raises(ZeroLead):
        inverse_series_newton([], 3, p)


def test_divrem_symbols_are_declared_exported_and_typed():
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
    assert "Errors of the eighteen" in header
    assert "zk_upoly_divrem(context<F>()" in mirror and "zk_upoly_inverse_series(context<F>()" in mirror
    assert "std::pair<UnivariatePolynomial, UnivariatePolynomial> divrem(const UnivariatePolynomial &b) const" in mirror
    assert ("fn zk_upoly_divrem(ctx: *mut zk_ctx, a: *const zk_upoly, b: *const zk_upoly, out_q: *mut *mut zk_upoly, "
            "out_r: *mut *mut zk_upoly) -> i32;") in shim
    assert "fn zk_upoly_inverse_series(ctx: *mut zk_ctx, f: *const zk_upoly, k: u64, out: *mut *mut zk_upoly) -> i32;" in shim
    impl = shim[shim.index("impl<F: GpuField> UnivariatePolynomial<F> {"):]
    assert re.search(r"pub fn divrem\(&self, b: &Self\) -> Result<\(Self, Self\), &'static str> \{", impl)
    assert re.search(r"pub fn inverse_series\(&self, k: u64\) -> Result<Self, &'static str> \{", impl)
    for name in ("divmod", "__divmod__", "__floordiv__", "__mod__", "inverse_series"):
        assert hasattr(zk_amd.UnivariatePolynomial, name), name
    assert hasattr(zk_amd, "upoly_divrem_host") and hasattr(zk_amd, "upoly_inverse_series_host")
    for switch in ("ZK_UPOLY_DIVREM_DIRECT_MAX", "ZK_UPOLY_DIVREM_LINEAR"):
        assert switch in header and switch in open(os.path.join(ROOT, "INTEGRATION.md")).read(), switch


def test_divrem_argument_checks_need_no_device():
    q, r, h = c.c_void_p(), c.c_void_p(), c.c_void_p()
    out = np.zeros((4, 4), dtype=np.uint64)
    p = out.ctypes.data_as(c.POINTER(c.c_uint64))
    assert lib.zk_upoly_divrem(None, None, None, c.byref(q), c.byref(r)) == BAD
    assert lib.zk_upoly_inverse_series(None, None, 3, c.byref(h)) == BAD
    assert lib.zk_upoly_divrem_host(None, p, 3, p, 2, p, p) == BAD
    assert lib.zk_upoly_inverse_series_host(None, p, 3, 2, p) == BAD
    assert lib.zk_bench_upoly_divrem(None, None, None, 0, 1, None) == BAD
    ctx = c.c_void_p()
    if lib.zk_ctx_create(zk_amd.BN254_FR, 0, c.byref(ctx)) != 0:
        return   # no device: a context cannot be made, and every other check needs one
    try:
        assert lib.zk_upoly_divrem_host(ctx, p, 3, p, 0, p, p) == BAD        # lb = 0
        assert lib.zk_upoly_divrem_host(ctx, p, 3, None, 2, p, p) == BAD
        assert lib.zk_upoly_divrem_host(ctx, None, 3, p, 2, p, p) == BAD
        # the length rule on short buffers, before anything is read: BN254, k = 2^28 needs 2^29-point transforms
        assert lib.zk_upoly_divrem_host(ctx, p, (1 << 28) + 2, p, 3, p, p) == UNSUP
        assert lib.zk_upoly_inverse_series_host(ctx, p, 3, 1 << 28, p) == UNSUP
    finally:
        lib.zk_ctx_destroy(ctx)


def test_divrem_without_gpu_fails_loudly():
    if not _no_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ZkError) as e:
        zk_amd.upoly_divrem_host(zk_amd.Context(zk_amd.BN254_FR, 0), np.zeros((3, 4), dtype=np.uint64), np.ones((2, 4), dtype=np.uint64))
    assert e.value.code == -22   # ZK_ERR_NO_DEVICE


def test_cpp_divrem_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_upoly_divrem")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_upoly_divrem.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    if not _no_gpu():
        pytest.skip("GPU present: run by tests/test_gpu_upoly_divrem.py")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr
