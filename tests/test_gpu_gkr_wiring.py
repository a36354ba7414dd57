"""GPU: the kernels that belong to the GKR driver alone -- k_gkr_phase<1|2>, k_gkr_phase{1,2}_heavy, k_eq_split, k_eq_halves / k_eq_outer,
k_gkr_wiring_eval, k_gkr_forward, the tree digests -- on wiring with prescribed CSR row lengths (tests/gkr_wiring.py: rows at 255..258
entries, rows straddling and ending on the 256-entry chunks, workgroups without entries, heavy rows between light ones), on extreme
layer shapes and on eq tables large enough for the sliced halves, on every field.  Small circuits are bit-exact against the big-int
definition (oracle/gkr_ref.py); the large ones go through tests/gkr_oracle_check.py (C oracle primitives only) and zk_gkr_verify; eq
tables are compared whole with orc.eq_table."""
import os
import random
import sys
import time

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from oracle import gkr_ref
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import gkr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gkr_wiring as gw  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from gkr_oracle_check import check_proof  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
_ctx = {}


def ctx_for(field):
    if field not in _ctx:
        _ctx[field] = zk_amd.Context(field, 0)
    return _ctx[field]


def upload_circuit(c, layers):
    circ = gkr.Circuit(c)
    for lo, li, op, left, right in layers:
        circ.add_layer(lo, li, op, left, right)
    return circ


def first_diff(got, want):
    """'' when the lists are equal, else where they first differ (an assertion message a reader can act on)"""
    if len(got) != len(want):
        return f"length {len(got)} != {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"element {i} of {len(want)}: got {g:#x}, want {w:#x} ({sum(a != b for a, b in zip(got, want))} differ)"
    return ""


def input_table(field, kind, n, seed):
    p = orc.modulus(field)
    if kind == "random":
        rng = random.Random(seed)
        return [rng.randrange(p) for _ in range(n)]
    if kind == "structured":   # whole tables of worst-case Montgomery limbs (tests/field_corpus.py)
        vals = worst_case_values(p, FIELDS.index(field), n)
        assert len(vals) == n
        return vals
    assert kind == "p-1"
    return [p - 1] * n


def check_bit_exact(field, layers, inputs, seed):
    """evaluate, prove and verify on the GPU against the model: outputs and proof element by element, accept, reject the middle element"""
    c = ctx_for(field)
    p = orc.modulus(field)
    as_lists = [(lo, li, op.tolist(), left.tolist(), right.tolist()) for lo, li, op, left, right in layers]
    t0 = time.perf_counter()
    want_out, want_proof = gkr_ref.gkr_prove(field, as_lists, inputs, seed)
    t_model = time.perf_counter() - t0
    t0 = time.perf_counter()
    circ = upload_circuit(c, layers)
    x = MLE.new(c, layers[-1][1], orc.from_ints(field, inputs))
    d = first_diff(orc.to_ints(field, circ.evaluate(x).evaluation_slice()), want_out)
    assert not d, f"evaluate: {d}"
    out, proof = gkr.gkr_prove(circ, x, seed)
    d = first_diff(orc.to_ints(field, out.evaluation_slice()), want_out)
    assert not d, f"prove outputs: {d}"
    d = first_diff(orc.to_ints(field, proof), want_proof)
    assert not d, f"proof: {d}"
    assert gkr.gkr_verify(circ, x, out, seed, proof)
    mid = len(want_proof) // 2
    bad = proof.copy()
    bad[mid] = orc.from_int(field, want_proof[mid] + 1)
    assert not gkr.gkr_verify(circ, x, out, seed, bad), f"proof element {mid} changed, accepted"
    circ.free()
    print(f"big-int model {t_model:.2f} s, everything else {time.perf_counter() - t0:.3f} s")


def _seed(*parts):
    return bytes(random.Random(repr(parts)).randrange(256) for _ in range(32))


# ---- (12 -> 8) profile layers, bit-exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name,ops", gw.CASES)
def test_profile_layer_single_point(field, name, ops):
    """the depth-1 circuit [(12 -> 8 profile)]: E is one eq table (fe_mul29 in eq_factor_at)"""
    inputs = input_table(field, "random", 1 << gw.P_IN, seed=f"{name}{ops}{field}")
    check_bit_exact(field, [gw.profile_layer(name, ops)], inputs, _seed(name, ops, field))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("table", ["structured", "p-1"])
@pytest.mark.parametrize("name", ["threshold", "straddle"])
def test_profile_layer_worst_case_tables(field, name, table):
    """W of the profile layer made of worst-case Montgomery limbs, and of p - 1 everywhere"""
    inputs = input_table(field, table, 1 << gw.P_IN, seed=None)
    check_bit_exact(field, [gw.profile_layer(name)], inputs, _seed(name, table, field))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["threshold", "straddle", "heavy_between_light"])
def test_profile_layer_two_points(field, name):
    """[(2 -> 12 random), (12 -> 8 profile)]: the profile layer's E is alpha eq(u) + beta eq(v) (fe_dot2_29 in eq_factor_at)"""
    layers = [gw.random_layer(2, gw.P_OUT, seed=31 + field), gw.profile_layer(name)]
    inputs = input_table(field, "random", 1 << gw.P_IN, seed=f"two{name}{field}")
    check_bit_exact(field, layers, inputs, _seed("two", name, field))


# ---- extreme layer shapes, bit-exact ------------------------------------------------------------------------------------------------------
def _shape_two_rows():
    return [gw.layer(12, 1, [2048, 2048], [2048, 2048], "random", seed=51)]   # every row heavy, empty light CSR, one sumcheck round


def _shape_sparse():
    return [gw.random_layer(2, 12, seed=52), gw.random_layer(12, 12, seed=53)]   # 4 gates over 4096 rows


def _shape_tiny():
    return [gw.random_layer(0, 1, seed=54), gw.random_layer(1, 1, seed=55)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("shape", [_shape_two_rows, _shape_sparse, _shape_tiny], ids=["12to1", "2to12_12to12", "0to1_1to1"])
def test_extreme_layer_shapes(field, shape):
    layers = shape()
    inputs = input_table(field, "random", 1 << layers[-1][1], seed=f"{shape.__name__}{field}")
    check_bit_exact(field, layers, inputs, _seed(shape.__name__, field))


# ---- large circuits: the oracle-only checker and the library's verifier ------------------------------------------------------------------
def check_large(field, layers, input_seed, seed):
    """-> seconds spent in (host: circuit upload, CPU evaluation, check_proof; device: evaluate, prove, verify)"""
    c = ctx_for(field)
    t0 = time.perf_counter()
    circ = upload_circuit(c, layers)
    t_host = time.perf_counter() - t0
    x = MLE.random(c, layers[-1][1], input_seed)
    xs = x.evaluation_slice()
    t0 = time.perf_counter()
    ev = circ.evaluate(x)
    out, proof = gkr.gkr_prove(circ, x, seed)
    assert gkr.gkr_verify(circ, x, out, seed, proof)
    bad = proof.copy()
    mid = bad.shape[0] // 2
    bad[mid] = orc.add(field, bad[mid], orc.from_int(field, 1))
    assert not gkr.gkr_verify(circ, x, out, seed, bad)
    t_dev = time.perf_counter() - t0
    outs = out.evaluation_slice()
    t0 = time.perf_counter()
    w = xs
    for _, _, op, left, right in reversed(layers):   # orc.circuit_layer layer by layer
        w = orc.circuit_layer(field, op, left, right, w)
    assert np.array_equal(ev.evaluation_slice(), w), "evaluate differs from the CPU evaluation"
    assert np.array_equal(outs, w), "prove's outputs differ from the CPU evaluation"
    ok, why = check_proof(field, layers, xs, outs, seed, proof)
    assert ok, why
    assert not check_proof(field, layers, xs, outs, seed, bad)[0], f"proof element {mid} changed, accepted by the oracle-only checker"
    t_host += time.perf_counter() - t0
    circ.free()
    return t_host, t_dev


@pytest.mark.parametrize("field", FIELDS)
def test_skewed_wide_layer_through_checker_and_verifier(field):
    """[(17 -> 19 random), (19 -> 18 skewed)]: k_eq_split with sliced hi halves (11 and 12 bits), k_tree_level, workgroups of twenty
    chunks next to heavy rows and rows of 255 / 256 / 257 entries, a row of 70001"""
    layers = [gw.random_layer(17, 19, seed=61), gw.skewed_layer()]
    t_host, t_dev = check_large(field, layers, 0x5E + field, _seed("skewed", field))
    print(f"skewed 2^19-gate layer, field {field}: host {t_host:.2f} s, device calls {t_dev:.3f} s")


def test_eq_split_with_eight_lo_bits():
    """[(24 -> 10), (10 -> 10)]: log_out = 24 is the smallest layer at which eq_split_lo_bits leaves 7.  The cost is host work (building,
    sorting and hashing 2^24 gates, the CPU checker); both times are printed."""
    field = zk_amd.BN254_FR
    t0 = time.perf_counter()
    layers = [gw.random_layer(24, 10, seed=71), gw.random_layer(10, 10, seed=72)]
    t_build = time.perf_counter() - t0
    t_host, t_dev = check_large(field, layers, 0x24, _seed("lo8"))
    print(f"2^24-gate layer: host {t_build + t_host:.2f} s, device calls {t_dev:.3f} s")


# ---- zk_eq_table (k_eq_halves + k_eq_outer) against orc.eq_table -----------------------------------------------------------------------
EQ_KINDS = ("random", "zeros", "ones", "bits", "mixed")


def eq_point(field, m, kind):
    p = orc.modulus(field)
    rng = random.Random(f"{kind}{m}{field}")
    if kind == "random":
        return [rng.randrange(p) for _ in range(m)]
    if kind == "zeros":
        return [0] * m
    if kind == "ones":
        return [1] * m
    if kind == "bits":
        return [rng.randrange(2) for _ in range(m)]
    pool = worst_case_values(p, FIELDS.index(field), 64)
    pt = [0, 1, p - 1, pool[0], pool[1]] + [rng.choice([0, 1, p - 1] + pool) if rng.random() < 0.5 else rng.randrange(p) for _ in range(m - 5)]
    rng.shuffle(pt)
    return pt


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", EQ_KINDS)
@pytest.mark.parametrize("m", [13, 16, 17, 18, 21, 22])
def test_eq_table_large_and_degenerate_points(field, m, kind):
    """m >= 17: the strided loops of k_eq_halves take a second trip (half tables of 2^9 and more entries).  Points of 0 / 1 turn the
    table into an indicator, 0, 1 and p - 1 among random coordinates turn half of it into exact zeros."""
    c = ctx_for(field)
    pt = eq_point(field, m, kind)
    e = orc.from_ints(field, pt)
    got = gkr.eq_table(c, e)
    arr = got.evaluation_slice()
    got.free()
    if kind in ("zeros", "ones", "bits"):   # the indicator of the index whose binary digits are the point, MSB first
        idx = int("".join(str(b) for b in pt), 2)
        assert np.array_equal(arr[idx], orc.from_int(field, 1))
        assert np.flatnonzero(arr.any(axis=1)).tolist() == [idx]
    want = orc.eq_table(field, e)
    assert np.array_equal(arr, want)
    del arr, want
