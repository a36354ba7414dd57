"""Dense coefficient-form multilinear polynomials without a GPU: the tests' restatement of CoeffMultilinearPolynomial::interpolate
(tests/cmle_ref.py, coefficient_form.rs:200-216) agrees with its fast form for every length 0..40 in every field, reproduces the
reference KAT, the new error code has the reference's text, and the new entry points are declared, typed and check their arguments
before any device work."""
import os
import subprocess
import sys

import pytest

import zk_amd
from zk_amd import _lib
from zk_amd._lib import c, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cmle_ref import evaluate_slice, interpolate_fast, interpolate_literal, to_bytes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
NAMES = ["zk_cmle_upload", "zk_cmle_download", "zk_cmle_n_vars", "zk_cmle_free", "zk_cmle_interpolate", "zk_cmle_interpolate_host",
         "zk_cmle_to_evaluation", "zk_cmle_evaluate", "zk_cmle_to_bytes", "zk_bench_cmle"]
BAD_ARG = -20


def _modulus(field):
    return int(zk_amd.modulus(field))


@pytest.mark.parametrize("field", FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def test_literal_and_fast_models_agree(field):
    p = _modulus(field)
    for length in range(41):
        vals = [(0x9E3779B97F4A7C15 * (i + 1) + length) ** 3 % p for i in range(length)]
        if length % 3 == 0:
            vals = [(p - 1 - v) % p for v in vals]   # values near p as well
        n, lit = interpolate_literal(vals, p)
        m, dense = interpolate_fast(vals, p)
        assert n == m
        assert sorted(lit) == list(range(len(dense)))   # every key present, zeros included
        assert [lit[k] for k in range(len(dense))] == dense, length
    assert interpolate_literal([], p) == (0, {}) and interpolate_fast([], p) == (0, [])
    assert interpolate_literal([7], p) == (1, {0: 7, 1: p - 7})   # the len == 1 rule: n_vars 1


@pytest.mark.parametrize("field", FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def test_reference_interpolation_kat(field):
    """test_interpolation (coefficient_form.rs:1105-1137): y = [2, 4, 8, 3] -> 2 + 6a + 2b - 7ab"""
    p = _modulus(field)
    n, dense = interpolate_fast([2, 4, 8, 3], p)
    assert n == 2 and dense == [2, 6, 2, p - 7]
    assert interpolate_literal([2, 4, 8, 3], p) == (2, {0: 2, 1: 6, 2: 2, 3: p - 7})
    for pt, want in [([0, 0], 2), ([0, 1], 4), ([1, 0], 8), ([1, 1], 3)]:
        assert evaluate_slice(n, dense, pt, p) == want
    assert evaluate_slice(n, dense, [1, 1, 5], p) == 3   # extra assignments are ignored
    with pytest.raises(ValueError):
        evaluate_slice(n, dense, [1], p)
    b = to_bytes(n, dense)
    assert len(b) == 4 + 40 * 4 and b[:4] == b"\0\0\0\2" and b[4:12] == bytes(8) and b[12:44] == (2).to_bytes(32, "big")


def test_eval_assignment_error_has_the_reference_text():
    text = lib.zk_strerror(-12)
    text = text.decode() if isinstance(text, bytes) else text
    assert text == "evaluate requires an assignment for every variable"
    assert "ZK_ERR_EVAL_ASSIGNMENT = -12" in open(os.path.join(ROOT, "include", "zk_amd.h")).read()


def test_cmle_symbols_are_declared_exported_and_typed():
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(lib, n) and n in _lib._sig, n
        assert getattr(lib, n).restype is c.c_int32
    assert lib.zk_abi_version() == 6
    for name in ["DeviceCoeffMultilinear", "cmle_interpolate_host"]:
        assert name in zk_amd.api.__all__ and hasattr(zk_amd, name)
    assert hasattr(zk_amd.CoeffMultilinearPolynomial, "interpolate")


def test_cmle_argument_checks_need_no_device():
    h = c.c_void_p()
    nv = c.c_uint64()
    out = (c.c_uint64 * 4)()
    assert lib.zk_cmle_upload(None, 0, None, 0, c.byref(h)) == BAD_ARG
    assert lib.zk_cmle_download(None, None, out) == BAD_ARG
    assert lib.zk_cmle_n_vars(None, c.byref(nv)) == BAD_ARG
    assert lib.zk_cmle_interpolate(None, None, c.byref(h)) == BAD_ARG
    assert lib.zk_cmle_interpolate_host(None, None, 0, c.byref(nv), None) == BAD_ARG
    assert lib.zk_cmle_to_evaluation(None, None, c.byref(h)) == BAD_ARG
    assert lib.zk_cmle_evaluate(None, None, None, 0, out) == BAD_ARG
    assert lib.zk_cmle_to_bytes(None, None, None) == BAD_ARG
    assert lib.zk_bench_cmle(None, 0, None, None, None, 0, 1, None) == BAD_ARG
    assert lib.zk_cmle_free(None, None) == 0   # freeing nothing is no error


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_cmle")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_cmle.cpp"), "-L" + lib_dir,
                    "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: run by tests/test_gpu_cmle.py")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr
