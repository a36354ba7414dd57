"""The algebra of coefficient-form multilinear polynomials without a GPU: the tests' dict model (tests/cmle_algebra_ref.py) reproduces
the vectors of the reference's own test module (coefficient_form.rs:691-1000, :1192-1245; the integers are the unreduced ones, our
moduli being 254 bits and more), the two new error codes carry the reference's texts, and the new entry points are declared, exported,
typed and check their arguments before any device work."""
import os
import subprocess
import sys

import pytest

import zk_amd
from zk_amd import _lib
from zk_amd._lib import c, lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cmle_algebra_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
IDS = ["bn254", "bls12_381", "bls12_377"]
NAMES = ["zk_cmle_fixed_mask", "zk_cmle_len", "zk_cmle_partial_evaluate", "zk_cmle_relabel", "zk_cmle_scalar_multiply", "zk_cmle_add",
         "zk_cmle_mul", "zk_bench_cmle_algebra"]
BAD_ARG = -20
T, F = True, False


def _modulus(field):
    return int(zk_amd.modulus(field))


def _poly_5ab_7bc_8d(p):   # :691-702
    return ref.new(4, [(5, [T, T, F, F]), (7, [F, T, T, F]), (8, [F, F, F, T])], p)


def test_get_variable_indexes_matches_the_reference():
    """test_get_variable_indexes :638-689"""
    for sel in ([F, F, F, F], [T, F, T, F]):
        with pytest.raises(ValueError, match="only select single variable"):
            ref.get_variable_indexes(4, sel)
    with pytest.raises(ValueError, match="selector array len"):
        ref.get_variable_indexes(4, [T, F, F])
    assert ref.get_variable_indexes(4, [T, F, F, F]) == [1, 3, 5, 7, 9, 11, 13, 15]
    assert ref.get_variable_indexes(4, [F, T, F, F]) == [2, 3, 6, 7, 10, 11, 14, 15]
    assert ref.get_variable_indexes(4, [F, F, T, F]) == [4, 5, 6, 7, 12, 13, 14, 15]
    assert ref.get_variable_indexes(4, [F, F, F, T]) == [8, 9, 10, 11, 12, 13, 14, 15]


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_partial_evaluate_vectors(field):
    p = _modulus(field)
    poly = _poly_5ab_7bc_8d(p)
    assert poly == (4, {3: 5, 6: 7, 8: 8})
    assert ref.partial_evaluate(poly, [], p) == poly                                           # :704-709
    q = ref.partial_evaluate(poly, [([F, T, F, F], 3), ([T, F, F, F], 2)], p)                  # :711-730  30 + 21c + 8d
    assert q == (4, {0: 30, 4: 21, 8: 8})
    assert ref.partial_evaluate(q, [([F, F, T, F], 2)], p) == (4, {0: 72, 8: 8})               # :732-745  72 + 8d
    every = [([T, F, F, F], 2), ([F, T, F, F], 4), ([F, F, T, F], 3), ([F, F, F, T], 5)]
    assert ref.partial_evaluate(poly, every, p) == (4, {0: 164})                               # :748-771
    assert ref.partial_evaluate(poly, every[:1] + [([T, F, F, F], 3)] + every[1:], p) == (4, {0: 164})   # :773-800 the first a counts
    assert ref.partial_evaluate(poly, [([T, F, F, F, F], 3)], p) == poly                       # :802-809 over-long: ignored
    assert ref.evaluate_slice(poly, [2, 4, 3, 5], p) == 164 and ref.evaluate_slice(poly, [2, 4, 3, 5, 8], p) == 164   # :818-840
    with pytest.raises(ValueError, match="selector array len"):
        ref.partial_evaluate(poly, [([T, F, F], 3)], p)
    with pytest.raises(ValueError, match="only select single variable"):
        ref.partial_evaluate(poly, [([T, T, F, F], 3)], p)


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_relabel_vectors(field):
    """test_poly_relabelling :1191-1245 and the helpers' own vectors :1139-1189"""
    p = _modulus(field)
    poly = ref.new(4, [(2, [T, T, F, F]), (3, [F, F, T, T]), (5, [T, F, T, T]), (6, [F, T, F, T])], p)
    q = ref.partial_evaluate(poly, [([F, T, F, F], 1), ([F, F, T, F], 1)], p)
    assert q == (4, {1: 2, 8: 9, 9: 5})
    assert ref.relabel(q, p) == (2, {1: 2, 2: 9, 3: 5})                                         # 2a + 9b + 5ab
    one = (0, {0: 1})
    assert ref.relabel(one, p) == one
    assert ref.variable_presence_vector(ref.new(3, [(3, [T, F, F]), (2, [F, F, T])], p)) == [T, F, T]
    mi = ref.mapping_instruction_from_variable_presence
    assert mi([T, F, F, T]) == [(3, 1)] and mi([T, F, F, T, T]) == [(3, 1), (4, 2)] and mi([F, F, T, T]) == [(2, 0), (3, 1)]
    assert mi([T, T]) == [] and mi([F, F]) == [] and mi([F, T, F, F, T, F]) == [(1, 0), (4, 1)]


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_mul_add_and_scalar_vectors(field):
    p = _modulus(field)
    pq = ref.mul(ref.new(2, [(5, [T, T])], p), ref.new(1, [(6, [T])], p), p)                    # :884-897  5ab * 6c
    assert pq == (3, {7: 30})
    pq = ref.mul(ref.new(3, [(3, [T, F, T]), (2, [T, T, F])], p), ref.new(2, [(7, [T, T])], p), p)   # :899-921
    assert pq == (5, {27: 14, 29: 21})
    a = ref.new(4, [(2, [T, F, F, F]), (3, [F, T, T, F]), (6, [F, F, F, T])], p)                # :924-977 the "crazy" case
    b = ref.new(4, [(4, [T, F, F, F]), (5, [F, T, T, F]), (2, [F, F, F, T])], p)
    assert ref.mul(a, b, p) == (8, {17: 8, 97: 10, 129: 4, 22: 12, 102: 15, 134: 6, 24: 24, 104: 30, 136: 12})
    three = ref.mul(ref.mul(ref.new(2, [(2, [T, F]), (3, [F, T])], p), ref.new(1, [(4, [T])], p), p), ref.new(1, [(5, [T])], p), p)
    assert three == (4, {13: 40, 14: 60})                                                       # :979-999
    poly = _poly_5ab_7bc_8d(p)
    twice = (4, {3: 10, 6: 14, 8: 16})
    assert ref.add(poly, poly, p) == twice                                                      # :842-857
    assert ref.scalar_multiply(poly, 2, p) == twice and ref.mul(poly, (0, {0: 2}), p) == twice  # :859-881
    assert ref.mul(poly, (0, {0: 1}), p) == poly and ref.add(poly, (0, {}), p) == poly          # :1001-1015 the two identities
    assert ref.add((0, {}), poly, p) == poly


def test_selector_errors_have_the_reference_texts():
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    for code, name, text in [(-13, "ZK_ERR_SELECTOR_LEN", ref.SELECTOR_LEN_TEXT), (-14, "ZK_ERR_SELECTOR_SINGLE", ref.SELECTOR_SINGLE_TEXT)]:
        got = lib.zk_strerror(code)
        assert (got.decode() if isinstance(got, bytes) else got) == text
        assert f"{name} = {code}" in header


def test_algebra_symbols_are_declared_exported_and_typed():
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and hasattr(lib, n) and n in _lib._sig, n
        assert getattr(lib, n).restype is c.c_int32
    assert lib.zk_abi_version() == 6
    for method in ["partial_evaluate", "relabel", "scalar_multiply", "__add__", "__mul__", "fixed_mask"]:
        assert hasattr(zk_amd.DeviceCoeffMultilinear, method), method
    assert "stay with the host class" not in zk_amd.DeviceCoeffMultilinear.__doc__
    assert "393-395" in zk_amd.DeviceCoeffMultilinear.__doc__   # the Mul divergence is stated where a user reads it
    hpp = open(os.path.join(ROOT, "zk_amd", "host", "zk.hpp")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for n in NAMES[:-1]:
        assert n + "(" in hpp and "fn " + n + "(" in shim, n


def test_algebra_argument_checks_need_no_device():
    h = c.c_void_p()
    m = c.c_uint64()
    s = (c.c_uint64 * 4)()
    ms = c.c_double()
    assert lib.zk_cmle_fixed_mask(None, c.byref(m)) == BAD_ARG
    assert lib.zk_cmle_len(None, c.byref(m)) == BAD_ARG
    assert lib.zk_cmle_partial_evaluate(None, None, None, None, None, 0, c.byref(h)) == BAD_ARG
    assert lib.zk_cmle_relabel(None, None) == BAD_ARG
    assert lib.zk_cmle_scalar_multiply(None, None, s, c.byref(h)) == BAD_ARG
    assert lib.zk_cmle_add(None, None, None, c.byref(h)) == BAD_ARG
    assert lib.zk_cmle_mul(None, None, None, c.byref(h)) == BAD_ARG
    assert lib.zk_bench_cmle_algebra(None, 0, None, None, None, None, None, 0, 1, c.byref(ms)) == BAD_ARG


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_cmle_algebra")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_cmle_algebra.cpp"), "-L" + lib_dir,
                    "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    import torch

    if torch.cuda.is_available():
        return   # a device is present: tests/test_gpu_cmle_algebra.py runs the program
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr
