"""UnivariatePolynomial without a GPU: the zk_upoly_* symbols are exported and typed, argument checks answer before any device
work, the calls fail loudly (no fallback) without a device, the C++ mirror compiles, and the Rust shim has the reference's
signatures (univariate_poly.rs:16-40,186-209)."""
import os
import re
import subprocess

import numpy as np
import pytest

import zk_amd
from zk_amd import _lib
from zk_amd._lib import ZkError, c, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")
NAMES = ["zk_upoly_upload", "zk_upoly_len", "zk_upoly_download", "zk_upoly_free", "zk_upoly_mul", "zk_upoly_evaluate",
         "zk_upoly_mul_host"]


def _no_gpu():
    import torch

    return not torch.cuda.is_available()


def test_upoly_symbols_are_declared_exported_and_typed():
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in _lib._sig, n
        assert getattr(lib, n).restype is c.c_int32
    assert lib.zk_abi_version() == 6


def test_upoly_argument_checks_need_no_device():
    h = c.c_void_p()
    out = c.c_uint64()
    assert lib.zk_upoly_upload(None, None, 0, c.byref(h)) == -20
    assert lib.zk_upoly_len(None, c.byref(out)) == -20
    assert lib.zk_upoly_mul(None, None, None, c.byref(h)) == -20
    assert lib.zk_upoly_evaluate(None, None, None, None) == -20
    assert lib.zk_upoly_download(None, None, None) == -20
    assert lib.zk_upoly_mul_host(None, None, 0, None, 0, None) == -20
    assert lib.zk_upoly_free(None, None) == 0   # freeing nothing is fine, like zk_mle_free


def test_upoly_without_gpu_fails_loudly():
    if not _no_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ZkError) as e:
        zk_amd.UnivariatePolynomial.new(zk_amd.Context(zk_amd.BN254_FR, 0), np.zeros((3, 4), dtype=np.uint64))
    assert e.value.code == -22   # ZK_ERR_NO_DEVICE


def test_cpp_upoly_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_upoly")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_upoly.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    if not _no_gpu():
        pytest.skip("GPU present: run by tests/test_gpu_upoly.py")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr


def test_rust_shim_has_the_reference_signatures():
    src = open(SHIM).read()
    impl = src[src.index("impl<F: GpuField> UnivariatePolynomial<F> {"):]
    assert re.search(r"pub fn new\(coefficients: Vec<F>\) -> Self \{", impl)
    assert re.search(r"pub fn coefficients\(&self\) -> &\[F\] \{", impl)
    assert re.search(r"pub fn evaluate\(&self, x: &F\) -> F \{", impl)
    mul = src[src.index("impl<F: GpuField> std::ops::Mul for &UnivariatePolynomial<F> {"):]
    assert re.match(r"impl<F: GpuField> std::ops::Mul for &UnivariatePolynomial<F> \{\n    type Output = UnivariatePolynomial<F>;\n"
                    r"    fn mul\(self, other: Self\) -> Self::Output \{", mul)
    assert "zk_upoly_mul(" in mul[:600]
    for derive in ("Clone for UnivariatePolynomial<F>", "PartialEq for UnivariatePolynomial<F>", "fmt::Debug for UnivariatePolynomial<F>"):
        assert "impl<F: GpuField> " + derive in src, derive
