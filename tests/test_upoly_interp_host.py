"""UnivariatePolynomial interpolation and Add without a GPU: the new symbols are declared, exported and typed, argument checks
answer before any device work, ZK_ERR_PANIC_INVERSE has its text, the C++ mirror compiles and fails loudly, the Rust shim carries
the reference's signatures (univariate_poly.rs:43-80, :157-184), and the tests' Python restatement of Lagrange interpolation
(tests/interp_ref.py) reproduces the reference's KATs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from zk_amd import _lib
from zk_amd._lib import ZkError, c, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interp_ref import RefPanic, add, lagrange, lagrange_literal  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")
NAMES = ["zk_upoly_add", "zk_upoly_interpolate", "zk_upoly_interpolate_xy", "zk_upoly_interpolate_host", "zk_upoly_interpolate_xy_host",
         "zk_bench_upoly_interp"]


def _no_gpu():
    import torch

    return not torch.cuda.is_available()


def test_interp_symbols_are_declared_exported_and_typed():
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in _lib._sig, n
        assert getattr(lib, n).restype is c.c_int32
    assert lib.zk_abi_version() == 6
    assert hasattr(zk_amd.UnivariatePolynomial, "interpolate") and hasattr(zk_amd.UnivariatePolynomial, "interpolate_xy")
    assert hasattr(zk_amd, "upoly_interpolate_host")


def test_interp_argument_checks_need_no_device():
    h = c.c_void_p()
    assert lib.zk_upoly_add(None, None, None, c.byref(h)) == -20
    assert lib.zk_upoly_interpolate(None, None, c.byref(h)) == -20
    assert lib.zk_upoly_interpolate_xy(None, None, None, c.byref(h)) == -20
    assert lib.zk_upoly_interpolate_host(None, None, 0, None) == -20
    assert lib.zk_upoly_interpolate_xy_host(None, None, 0, None, 0, None) == -20
    assert lib.zk_bench_upoly_interp(None, None, None, 1, None) == -20


def test_panic_inverse_has_its_text():
    text = lib.zk_strerror(-11)
    text = text.decode() if isinstance(text, bytes) else text
    assert "inverse().unwrap()" in text and "repeated x" in text
    assert "ZK_ERR_PANIC_INVERSE = -11" in open(os.path.join(ROOT, "include", "zk_amd.h")).read()


def test_interp_without_gpu_fails_loudly():
    if not _no_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ZkError) as e:
        zk_amd.UnivariatePolynomial.interpolate(zk_amd.Context(zk_amd.BN254_FR, 0), np.zeros((3, 4), dtype=np.uint64))
    assert e.value.code == -22   # ZK_ERR_NO_DEVICE


def test_cpp_interp_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_upoly_interp")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_upoly_interp.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    if not _no_gpu():
        pytest.skip("GPU present: run by tests/test_gpu_upoly_interp.py")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr


def test_rust_shim_has_the_reference_signatures():
    src = open(SHIM).read()
    impl = src[src.index("impl<F: GpuField> UnivariatePolynomial<F> {"):]
    assert re.search(r"pub fn interpolate\(ys: Vec<F>\) -> Self \{", impl)
    assert re.search(r"pub fn interpolate_xy\(xs: Vec<F>, ys: Vec<F>\) -> Self \{", impl)
    add_impl = src[src.index("impl<F: GpuField> std::ops::Add for &UnivariatePolynomial<F> {"):]
    assert re.match(r"impl<F: GpuField> std::ops::Add for &UnivariatePolynomial<F> \{\n    type Output = UnivariatePolynomial<F>;\n"
                    r"    fn add\(self, other: Self\) -> Self::Output \{", add_impl)
    assert "zk_upoly_add(" in add_impl[:600]


def test_python_restatement_reproduces_the_reference_kats():
    """test_polynomial_interpolation (:322-350) in the reference's own field, F_17, and over a large prime; Add (:266-293)"""
    for p in (17, (1 << 61) - 1):
        for f in (lagrange_literal, lagrange):
            assert f([0, 1], [0, 2], p) == [0, 2]
            assert f([0, 1, 2], [5, 7, 13], p) == [5, 0, 2]
            assert f([5, 7, 9, 1], [565, 1631, 3537, -7], p) == [0, p - 12, 0, 5]
            got = f([0, 1, 3, 4, 5, 8], [12, 48, 3150, 11772, 33452, 315020], p)
            assert got == [v % p for v in [12, 25, 18, 24, 12, 8]] if p == 17 else got == [12, 8, 1, 7, 12, 8]
            assert f([1, 2], [], p) == [] and f([], [1, 2], p) == []
            assert f([4, 5, 6], [9], p) == lagrange_literal([4, 5, 6], [9], p)
    assert add([], [], 17) == [] and add([], [0, 2], 17) == [0, 2] and add([0, 2], [], 17) == [0, 2]
    assert add([4, 3, 2], [3, 4, 0, 4], 17) == [7, 7, 2, 4] == add([3, 4, 0, 4], [4, 3, 2], 17)
    with pytest.raises(RefPanic):
        lagrange_literal([1, 2, 1], [5, 6, 7], 17)
    assert lagrange_literal([1, 2, 2], [5], 17) == lagrange([1, 2, 2], [5], 17)   # repeats above m = 1: no panic
