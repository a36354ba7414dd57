"""GPU parity: the HIP path (through the C ABI) against the CPU oracle, bit for bit, on the same seeded inputs.

Layout follows the reference's own tests (evaluation_form.rs:106-203, product_poly.rs:91-197,
sumcheck/src/lib.rs:31-123, fft/src/lib.rs:63-83) and then widens to random tables, every fold position, edge
values, all three fields and the (k, D) grid.  Run with -m gpu on the MI355X box.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import ProductPoly, SumcheckProof, SumcheckProver, SumcheckVerifier, ZkError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
_ctx = {}


def ctx_for(field):
    if field not in _ctx:
        _ctx[field] = zk_amd.Context(field, 0)
    return _ctx[field]


def F(field, vals):
    return zk_amd.fe_from_ints(field, vals)


def ints(field, arr):
    p = zk_amd.modulus(field)
    return [v if v <= p // 2 else v - p for v in zk_amd.fe_to_ints(field, arr)]


def sum_elems(field, arr):
    return orc.sum_elems(field, np.asarray(arr).reshape(-1, 4))   # iter().sum::<F>() (prover.rs:53-54)


# ------------------------------------------------------------------ reference KATs through the GPU path
@pytest.mark.parametrize("field", FIELDS)
def test_ref_new_and_partial_evaluate_kats(field):
    c = ctx_for(field)
    with pytest.raises(ZkError, match="evaluation vec len should equal 2\\^n_vars"):   # evaluation_form.rs:112-119
        MLE.new(c, 2, F(field, [3, 1, 2]))
    with pytest.raises(ZkError, match="evaluation vec len should equal 2\\^n_vars"):
        MLE.new(c, 2, F(field, [3, 1]))
    MLE.new(c, 1, F(field, [3, 1]))
    t = MLE.new(c, 2, F(field, [3, 1, 2, 5]))
    assert ints(field, t.partial_evaluate(0, F(field, [5])).evaluation_slice()) == [-2, 21]   # :128-137
    assert ints(field, t.partial_evaluate(0, F(field, [0])).evaluation_slice()) == [3, 1]     # :139-146
    assert ints(field, t.partial_evaluate(0, F(field, [1])).evaluation_slice()) == [2, 5]
    p = MLE.new(c, 3, F(field, [0, 0, 0, 3, 0, 0, 2, 5]))                                     # 2ab + 3bc
    assert ints(field, p.partial_evaluate(1, F(field, [2, 3])).evaluation_slice()) == [18, 22]  # :149-171
    assert ints(field, p.evaluate(F(field, [2, 3, 4]))) == [48]                               # :181-202
    with pytest.raises(ZkError, match="evaluate must assign to all variables"):
        p.evaluate(F(field, [2, 3]))
    assert p.partial_evaluate(0, F(field, [])).evaluation_slice().shape == (8, 4)
    for bad in [(3, [1]), (0, [1, 2, 3, 4]), (2, [1, 2])]:                                    # reference panics
        with pytest.raises(ZkError, match="reference panics"):
            p.partial_evaluate(bad[0], F(field, bad[1]))


@pytest.mark.parametrize("field", FIELDS)
def test_ref_product_poly_kats(field):
    c = ctx_for(field)
    a, b = MLE.new(c, 2, F(field, [2, 8, 10, 14])), MLE.new(c, 2, F(field, [2, 8, 10, 22]))
    with pytest.raises(ZkError, match="share the same number of variables"):                  # product_poly.rs:98-111
        ProductPoly.new([a, MLE.new(c, 1, F(field, [3, 1]))])
    with pytest.raises(ZkError, match="empty polynomials"):
        ProductPoly.new([])
    pp = ProductPoly.new([a, b])
    assert ints(field, pp.prod_reduce()) == [4, 64, 100, 308]                                 # :179-196
    pe = pp.partial_evaluate(1, F(field, [10]))                                               # :154-176
    assert ints(field, pe.polynomials[0].evaluation_slice()) == [62, 50]
    assert ints(field, pe.polynomials[1].evaluation_slice()) == [62, 130]
    three = ProductPoly.new([a, b, MLE.new(c, 2, F(field, [3, 1, 2, 5]))])                    # :124-151
    pt = F(field, [1, 10])
    want = 1
    for q in three.polynomials:
        want = want * zk_amd.fe_to_int(field, q.evaluate(pt)) % zk_amd.modulus(field)
    assert zk_amd.fe_to_int(field, three.evaluate(pt)) == want
    with pytest.raises(ZkError, match="evaluate must assign to all variables"):
        three.evaluate(F(field, [1]))


@pytest.mark.parametrize("field", FIELDS)
def test_ref_sumcheck_kats(field):
    c = ctx_for(field)
    p = ProductPoly.new([MLE.new(c, 3, F(field, [0, 0, 0, 3, 0, 0, 2, 5]))])
    proof = SumcheckProver(1).prove(p, zk_amd.fe_from_int(field, 10))                          # sumcheck/src/lib.rs:53-62
    assert ints(field, proof.round_polys[0]) == [3, 7]
    assert SumcheckVerifier.verify(p, proof) is True
    q = ProductPoly.new([MLE.new(c, 2, F(field, [3, 3, 5, 5])), MLE.new(c, 2, F(field, [0, 0, 0, 1]))])
    proof2 = SumcheckProver(2).prove(q, zk_amd.fe_from_int(field, 5))                          # :64-100
    assert ints(field, proof2.round_polys[0]) == [0, 5, 14]
    assert SumcheckVerifier.verify(q, proof2) is True
    proof3, ch = SumcheckProver(1).prove_partial(p, zk_amd.fe_from_int(field, 10))             # :102-112
    sub = SumcheckVerifier.verify_partial(field, proof3)
    assert np.array_equal(sub.challenges, ch)
    assert np.array_equal(p.evaluate(sub.challenges), sub.sum)
    bad = SumcheckProver(1).prove(p, zk_amd.fe_from_int(field, 12))                            # :114-122
    with pytest.raises(ZkError, match="claimed_sum != p\\(0\\) \\+ p\\(1\\)"):
        SumcheckVerifier.verify(p, bad)
    with pytest.raises(ZkError, match="require 1 round poly"):
        SumcheckVerifier.verify(p, SumcheckProof(proof.sum, proof.round_polys[:2]))


@pytest.mark.parametrize("field", [zk_amd.BLS12_377_FR, zk_amd.BN254_FR, zk_amd.BLS12_381_FR])
def test_ref_fft_roundtrip_kat(field):
    c = ctx_for(field)
    a = F(field, [0, 2, 34, 3434])                                                             # fft/src/lib.rs:78-82
    assert np.array_equal(zk_amd.ifft(c, zk_amd.fft(c, a)), a)


# ------------------------------------------------------------------ fold vs oracle
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n_vars", [1, 2, 3, 6, 7, 8, 9])   # 7: the first size with 64 pairs (k_fold_low / k_fold_run / k_fold_msb take over from k_fold)
def test_fold_every_position_and_length(field, n_vars):
    c = ctx_for(field)
    p = zk_amd.modulus(field)
    tab = orc.fill_random(field, 1000 + n_vars, 1 << n_vars)
    t = MLE.new(c, n_vars, tab)
    rng = random.Random(n_vars * 7 + field)
    for initial_var in range(n_vars):
        for n_assign in range(0, n_vars - initial_var + 1):
            asg = F(field, [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(n_assign)])
            got = t.partial_evaluate(initial_var, asg).evaluation_slice()
            assert np.array_equal(got, orc.mle_partial_evaluate(field, n_vars, tab, initial_var, asg))
    assert np.array_equal(t.evaluation_slice(), tab)   # input untouched


@pytest.mark.parametrize("field", FIELDS)
def test_fold_general_positions_through_the_run_kernel(field):
    """partial_evaluate at every initial_var of a 2^14 table (index bits 13..0): bits >= 6 take k_fold_run (wave-coalesced runs,
    block by block), the low six bits k_fold_low (one in-wave exchange); single and multiple assignments (each later assignment folds the SAME variable index
    of the shrunken table, evaluation_form.rs:54-72), edge challenges included.  Bit-exact vs the oracle."""
    c = ctx_for(field)
    p = zk_amd.modulus(field)
    n = 14
    tab = orc.fill_random(field, 1400 + field, 1 << n)
    t = MLE.new(c, n, tab)
    rng = random.Random(14 + field)
    for initial_var in range(n):
        for n_assign in (1, 2, 3, n - initial_var):
            if n_assign > n - initial_var:
                continue
            asg = F(field, [rng.choice([0, 1, p - 1, rng.randrange(p), rng.randrange(p)]) for _ in range(n_assign)])
            got = t.partial_evaluate(initial_var, asg).evaluation_slice()
            assert np.array_equal(got, orc.mle_partial_evaluate(field, n, tab, initial_var, asg)), (initial_var, n_assign)
    assert np.array_equal(t.evaluation_slice(), tab)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n_vars", [12, 16])
def test_msb_fold_evaluate_to_bytes_random(field, n_vars):
    c = ctx_for(field)
    tab = orc.fill_random(field, 2000 + n_vars, 1 << n_vars)
    t = MLE.new(c, n_vars, tab)
    r = orc.fill_random(field, 99, 1)
    assert np.array_equal(t.partial_evaluate(0, r).evaluation_slice(), orc.mle_partial_evaluate(field, n_vars, tab, 0, r))
    out = MLE.alloc(c, n_vars - 1)
    assert np.array_equal(t.fold_into(r[0], out).evaluation_slice(), orc.mle_partial_evaluate(field, n_vars, tab, 0, r))
    pt = orc.fill_random(field, 98, n_vars)
    assert np.array_equal(t.evaluate(pt), orc.mle_evaluate(field, n_vars, tab, pt))
    assert t.to_bytes() == orc.mle_to_bytes(field, n_vars, tab)


@pytest.mark.parametrize("field", FIELDS)
def test_fold_edge_values(field):
    c = ctx_for(field)
    p = zk_amd.modulus(field)
    n_vars = 8
    for fill in (0, p - 1, 1):
        tab = F(field, [fill] * (1 << n_vars))
        t = MLE.new(c, n_vars, tab)
        for rv in (0, 1, p - 1, 2, (p - 1) // 2):
            r = F(field, [rv])
            assert np.array_equal(t.partial_evaluate(0, r).evaluation_slice(),
                                  orc.mle_partial_evaluate(field, n_vars, tab, 0, r))
    # alternating extremes maximise the borrow / carry paths
    tab = F(field, [0 if i & 1 else p - 1 for i in range(1 << n_vars)])
    t = MLE.new(c, n_vars, tab)
    for iv in (0, n_vars - 1):
        r = F(field, [p - 1])
        assert np.array_equal(t.partial_evaluate(iv, r).evaluation_slice(),
                              orc.mle_partial_evaluate(field, n_vars, tab, iv, r))


@pytest.mark.parametrize("field", FIELDS)
def test_fill_random_matches_oracle_generator(field):
    c = ctx_for(field)
    t = MLE.random(c, 10, seed=0x5EED0002, first_index=12345)
    assert np.array_equal(t.evaluation_slice(), orc.fill_random(field, 0x5EED0002, 1 << 10, first_index=12345))


# ------------------------------------------------------------------ coefficient form -> evaluation form (the step before the path)
@pytest.mark.parametrize("field", FIELDS)
def test_ref_to_evaluation_form_kat_and_random(field):
    c = ctx_for(field)
    p2ab3bc = zk_amd.CoeffMultilinearPolynomial.new(field, 3, [(zk_amd.fe_from_int(field, 2), [True, True, False]),
                                                               (zk_amd.fe_from_int(field, 3), [False, True, True])])
    assert ints(field, p2ab3bc.to_evaluation_form(c).evaluation_slice()) == [0, 0, 0, 3, 0, 0, 2, 5]   # coefficient_form.rs:1322-1347
    with pytest.raises(ZkError, match="selector array len"):
        zk_amd.CoeffMultilinearPolynomial.new(field, 3, [(zk_amd.fe_from_int(field, 2), [True, True])])
    with pytest.raises(ZkError, match="more than specificed number of variables"):
        zk_amd.CoeffMultilinearPolynomial.new_with_coefficient(field, 2, {4: zk_amd.fe_from_int(field, 1)})
    # duplicate selectors are summed by ::new (:164-171)
    dup = zk_amd.CoeffMultilinearPolynomial.new(field, 2, [(zk_amd.fe_from_int(field, 2), [True, False]),
                                                           (zk_amd.fe_from_int(field, 5), [True, False])])
    assert ints(field, dup.to_evaluation_form(c).evaluation_slice()) == [0, 0, 7, 7]
    rng = random.Random(field)
    for n_vars, n_terms in [(1, 2), (2, 3), (4, 9), (5, 20), (8, 100), (9, 300), (11, 700), (13, 2000), (16, 65536)]:   # n mod 3 = 0, 1, 2
        keys = sorted(rng.sample(range(1 << n_vars), min(n_terms, 1 << n_vars)))
        coeffs = orc.fill_random(field, 2600 + n_vars, len(keys))
        poly = zk_amd.CoeffMultilinearPolynomial.new_with_coefficient(field, n_vars, {k: coeffs[i] for i, k in enumerate(keys)})
        got = poly.to_evaluation_form(c).evaluation_slice()
        if n_vars <= 13:
            assert np.array_equal(got, orc.coeff_to_evaluation(field, n_vars, keys, coeffs))
        else:   # dense 2^16: check through the MLE property instead of the O(4^n) oracle
            pt = orc.fill_random(field, 17, n_vars)
            ev = MLE.new(c, n_vars, got).evaluate(pt)
            acc = 0
            pm = zk_amd.modulus(field)
            rp = zk_amd.fe_to_ints(field, pt)
            cf = zk_amd.fe_to_ints(field, coeffs)
            # the table is the MLE of the polynomial: its value at a random point is sum_S c_S prod_{v in S} r_v
            for i, k in enumerate(keys):
                t, kk, v = cf[i], k, 0
                while kk:
                    if kk & 1:
                        t = t * rp[v] % pm
                    kk >>= 1
                    v += 1
                acc = (acc + t) % pm
            assert zk_amd.fe_to_int(field, ev) == acc


@pytest.mark.parametrize("field", FIELDS)
def test_to_evaluation_form_every_arity_and_term_class(field):
    """coefficient_form.rs:340-347 on the LDS-tiled passes (zeta_kernels.cuh): every n = 1..24 -- one partial tile below 11
    variables, the 11-bit first pass alone at 11, then 1..8-bit strided passes in every split up to 11 + 7 + 6 -- against the
    oracle's direct definition, with the term classes that exercise the first pass's tile logic: no term at all, the constant
    term only, the all-variables term only, all terms inside one 2^11 tile, terms in every tile, random."""
    c = ctx_for(field)
    rng = random.Random(1000 + field)
    for n_vars in range(1, 25):
        full = (1 << n_vars) - 1
        budget = max(2, min(300, (1 << 27) >> n_vars))   # oracle cost = 2^n * terms
        classes = {
            "none": [],
            "constant": [0],
            "all_variables": [full],
            "random": sorted(rng.sample(range(1 << n_vars), min(budget, 1 << n_vars))),
        }
        if n_vars >= 12:
            # table index = bit-reversed key: keys whose LOW n - 11 bits are fixed share the index's high bits, i.e. one tile
            hi_bits = rng.randrange(1 << (n_vars - 11))
            classes["one_tile"] = sorted({(rng.randrange(1 << 11) << (n_vars - 11)) | hi_bits for _ in range(min(budget, 40))})
            # ... and keys that only use the low n - 11 bits put one term at the START of many different tiles
            classes["tile_heads"] = sorted({rng.randrange(1 << (n_vars - 11)) for _ in range(min(budget, 40))})
        if n_vars <= 10:
            classes["dense"] = list(range(1 << n_vars))
        for name, keys in classes.items():
            if n_vars > 20 and name not in ("random", "one_tile"):
                continue   # (big tables: two classes keep the test in seconds)
            coeffs = orc.fill_random(field, 2700 + 31 * n_vars + len(keys), max(len(keys), 1))[:len(keys)]
            poly = zk_amd.CoeffMultilinearPolynomial.new_with_coefficient(field, n_vars, {k: coeffs[i] for i, k in enumerate(keys)})
            t = poly.to_evaluation_form(c)
            got = t.evaluation_slice()
            t.free()
            want = orc.coeff_to_evaluation(field, n_vars, keys, coeffs)
            assert np.array_equal(got, want), (n_vars, name)


def test_to_evaluation_form_tiled_equals_global_passes():
    """the round-4 form (memset + scatter + three index bits per launch, ZK_ZETA_GLOBAL=1) and the LDS-tiled passes give the
    same table on a dense-ish term list at 2^22 (child process: the switch is read once per process)"""
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import zk_amd\n"
        "f = zk_amd.BN254_FR; c = zk_amd.Context(f, 0)\n"
        "rng = np.random.default_rng(77); n = 22\n"
        "keys = np.unique(rng.integers(0, 1 << n, 1 << 15, dtype=np.uint64))\n"
        "co = zk_amd.MultiLinearPolynomial.random(c, 15, 99, 0).evaluation_slice()[:len(keys)]\n"
        "p = zk_amd.CoeffMultilinearPolynomial.new_with_coefficient(f, n, {int(k): co[i] for i, k in enumerate(keys)})\n"
        "t = p.to_evaluation_form(c)\n"
        "import hashlib; print('DIGEST', hashlib.sha256(t.evaluation_slice().tobytes()).hexdigest())\n"
    ) % ROOT
    outs = []
    for env in ({}, {"ZK_ZETA_GLOBAL": "1"}):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0])
    assert outs[0] == outs[1]


def _raw_coeff_to_evaluation(c, n_vars, keys, coeffs):
    """zk_coeff_to_evaluation on the caller's arrays as they are (duplicate keys included: the library sums them as the reference's BTreeMap does)"""
    from zk_amd._lib import c as C, check, lib, u64p

    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
    h = C.c_void_p()
    check(lib.zk_coeff_to_evaluation(c._h, n_vars, keys.ctypes.data_as(u64p), coeffs.ctypes.data_as(u64p), len(keys), C.byref(h)))
    return MLE(c, h)


_LONG_LIST_CHILD = r"""
import sys, hashlib
sys.path.insert(0, %r)
import numpy as np
import zk_amd
from zk_amd._lib import c as C, check, lib, u64p
f = zk_amd.BN254_FR
ctx = zk_amd.Context(f, 0)
for n, m in ((20, 1 << 16), (24, 1 << 16), (13, 1 << 14)):
    rng = np.random.default_rng(1000 + n)
    keys = rng.integers(0, 1 << n, m, dtype=np.uint64)          # unsorted, with repeats
    co = zk_amd.MultiLinearPolynomial.random(ctx, 16, 77 + n, 0).evaluation_slice()[:m]
    h = C.c_void_p()
    check(lib.zk_coeff_to_evaluation(ctx._h, n, keys.ctypes.data_as(u64p), co.ctypes.data_as(u64p), m, C.byref(h)))
    t = zk_amd.MultiLinearPolynomial(ctx, h)
    print("DIGEST", n, hashlib.sha256(t.evaluation_slice().tobytes()).hexdigest())
    t.free()
"""


def test_to_evaluation_form_long_term_lists_ordered_on_the_device():
    """coefficient_form.rs:340-347 with a LONG term list: from 4096 terms the list is uploaded as given and ordered on the device
    (zeta_sort.hip; the first pass sums runs of equal keys itself -- BTreeMap semantics, :164-171).  (a) 6000 terms over 2^12 keys (many
    repeats) against the oracle's direct definition; (b) 2^14 .. 2^16 unsorted terms with repeats at n = 13 / 20 / 24: the device-ordered
    table equals the host-ordered one bit for bit (child processes, ZK_ZETA_DEVICE_SORT_MIN moved either way)."""
    for field in FIELDS:
        c = ctx_for(field)
        n, m = 12, 6000
        rng = np.random.default_rng(12000 + field)
        keys = rng.integers(0, 1 << n, m, dtype=np.uint64)
        coeffs = orc.fill_random(field, 12345 + field, m)
        got = _raw_coeff_to_evaluation(c, n, keys, coeffs)
        assert np.array_equal(got.evaluation_slice(), orc.coeff_to_evaluation(field, n, keys, coeffs)), field
        got.free()
    outs = []
    for env in ({"ZK_ZETA_DEVICE_SORT_MIN": "0"}, {"ZK_ZETA_DEVICE_SORT_MIN": str(1 << 40)}, {}):
        r = subprocess.run([sys.executable, "-c", _LONG_LIST_CHILD % ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")])
    assert len(outs[0]) == 3 and outs[0] == outs[1] == outs[2]


def test_to_evaluation_form_every_arity_with_the_device_sort_forced():
    """the every-arity / term-class grid above with EVERY list ordered on the device (ZK_ZETA_DEVICE_SORT_MIN=0, child pytest): empty
    tiles, tile heads, one-tile lists and the constant term through k_term_indices + rocPRIM's radix sort + the permuted first pass"""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_to_evaluation_form_every_arity_and_term_class or test_ref_to_evaluation_form_kat_and_random"],
                       env=dict(os.environ, ZK_ZETA_DEVICE_SORT_MIN="0"), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ product / round sums vs oracle
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_prod_reduce_random(field, k):
    c = ctx_for(field)
    for n_vars in (0, 3, 5, 6, 10, 13):   # below 64 elements: k_prod_reduce; from 64: the wave-coalesced k_prod_reduce_run
        tabs = [orc.fill_random(field, 300 + f + 10 * n_vars, 1 << n_vars) for f in range(k)]
        pp = ProductPoly.new([MLE.new(c, n_vars, t) for t in tabs])
        assert np.array_equal(pp.prod_reduce(), orc.prod_reduce(field, n_vars, tabs)), n_vars


def oracle_round_sums(field, n_vars, tabs, D):
    out = []
    for t in range(D + 1):
        a = orc.from_int(field, t)[None, :]
        folded = [orc.mle_partial_evaluate(field, n_vars, tb, 0, a) for tb in tabs]
        out.append(sum_elems(field, orc.prod_reduce(field, n_vars - 1, folded)))
    return np.stack(out)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k,D", [(1, 1), (1, 3), (2, 1), (2, 2), (2, 4), (3, 3), (4, 4), (2, 0), (3, 6), (8, 2)])
@pytest.mark.parametrize("n_vars", [1, 5, 13])
def test_round_sums_grid(field, k, D, n_vars):
    c = ctx_for(field)
    tabs = [orc.fill_random(field, 400 + 10 * f + k, 1 << n_vars) for f in range(k)]
    pp = ProductPoly.new([MLE.new(c, n_vars, t) for t in tabs])
    assert np.array_equal(pp.round_sums(D), oracle_round_sums(field, n_vars, tabs, D))


def test_round_sums_lazy_reduction_worst_case():
    """all elements of VALUE p - 1, then the true worst case.  The wide accumulator sums products of STORED limbs (the Montgomery
    representation): the value p - 1 is stored as p - (R mod p) = 0.71 p, 0.79 p, 0.29 p (BN254, BLS12-381, BLS12-377), and kMaxLazy = 32
    such products reach a top word of 0, 4, 0 -- not the maximum.  The raw-limb tables const(M), M = p - 1 the largest representation
    (top word 1, 6, 0: the maximum), and const(O), O = 2^(bits - 1) - 1 with every 29-bit limb all ones, are the worst cases
    (tests/extreme_tables.py; tests/test_extreme_tables_host.py reproduces each figure)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import extreme_tables as et

    for field in FIELDS:
        c = ctx_for(field)
        p = zk_amd.modulus(field)
        n_vars = 14   # > 16 pairs per thread would need > 2048*256*16 pairs; the flush path is hit via lazy == kMaxLazy below
        tabs = [F(field, [p - 1]) .repeat(1 << n_vars, axis=0) for _ in range(2)]
        pp = ProductPoly.new([MLE.new(c, n_vars, t) for t in tabs])
        assert np.array_equal(pp.round_sums(2), oracle_round_sums(field, n_vars, tabs, 2))
        for name in ("const(M)", "const(O)"):
            tabs, closed = et.family(field, name, n_vars, 2)
            pp = ProductPoly.new([MLE.new(c, n_vars, t) for t in tabs])
            got = pp.round_sums(2)
            assert np.array_equal(got, oracle_round_sums(field, n_vars, tabs, 2)), (field, name)
            assert np.array_equal(got, et.elems(field, closed.round_sums(2))), (field, name)


_LAZY_CHILD = """
import os, sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(sys.path[0], "tests"))
import zk_amd
import extreme_tables as et
from oracle import binding as orc
checked = 0
for field in (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR):
    c = zk_amd.Context(field, 0)
    p = zk_amd.modulus(field)
    # the value p - 1 (stored as p - (R mod p)), then the raw-limb worst cases: M = p - 1 and the all-ones O as stored limbs
    for k, D, n, fill in [(k, D, n, fill) for fill in ("value p-1", "const(M)", "const(O)")
                          for k, D, n in ((2, 2, 15), (2, 2, 16), (3, 3, 15), (2, 1, 15), (2, 3, 15))]:
        if fill == "value p-1":
            tabs = [orc.from_ints(field, [p - 1]).repeat(1 << n, axis=0) for _ in range(k)]
        else:
            tabs = [t.copy() for t in et.family(field, fill, n, k)[0]]
        want = []
        for t in range(D + 1):
            a = orc.from_int(field, t)[None, :]
            folded = [orc.mle_partial_evaluate(field, n, tb, 0, a) for tb in tabs]
            acc = orc.sum_elems(field, orc.prod_reduce(field, n - 1, folded))   # iter().sum::<F>()
            want.append(acc)
        pp = zk_amd.ProductPoly.new([zk_amd.MultiLinearPolynomial.new(c, n, t) for t in tabs])
        assert np.array_equal(pp.round_sums(D), np.stack(want)), (field, k, D, n, fill)
        # and a whole proof: the fused rounds accumulate as many products per lane
        claimed = orc.add(field, want[0], want[1])
        rp, ch = orc.sumcheck_prove(field, n, tabs, D, claimed, False)
        proof, got_ch = zk_amd.SumcheckProver(D).prove_partial(pp, claimed)
        assert np.array_equal(proof.round_polys, rp) and np.array_equal(got_ch, ch), (field, k, D, n, fill)
        checked += 1
print("lazy ok", checked)
"""


def test_unreduced_accumulators_at_their_product_limit():
    """kMaxLazy products per lane before the one Montgomery reduction: a child process with ZK_ROUND_MIN_BLOCKS=1 makes the round
    kernels run with as FEW workgroups as the limit allows (2^14-2^15 pairs on 2-4 workgroups: every thread at the limit), on all three
    fields, round sums and whole proofs against the oracle.  Three fills: the VALUE p - 1, whose stored limbs p - (R mod p) are only
    0.71 p / 0.79 p / 0.29 p and give the wide accumulator a top word of 0 / 4 / 0 (and an arbitrary pattern of 29-bit limbs, so the
    carry-free column sums stay near their average); the raw representation M = p - 1, the largest possible unreduced sums with the
    top word at its maximum 1 / 6 / 0; and the raw all-ones representation O, every 29-bit column sum at its maximum.  The child also
    switches the quad and pipelined kernels off: tests/test_gpu_extreme_tables.py puts the same tables through those."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _LAZY_CHILD % root], env=dict(os.environ, ZK_ROUND_MIN_BLOCKS="1", ZK_QUAD_MAX_PAIRS="0",
                                                                           ZK_PIPE_MAX_PAIRS="0", ZK_LEAD_MIN_PAIRS="1", ZK_SKIP1_MIN_PAIRS="1"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "lazy ok 45" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ prover vs oracle (bit-exact transcript)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k,D,n_vars", [(1, 1, 12), (2, 2, 12), (3, 3, 10), (2, 1, 7), (1, 3, 6), (4, 4, 8), (2, 2, 1),
                                        (2, 2, 2), (2, 5, 6), (1, 0, 4), (2, 3, 9), (5, 2, 6), (8, 8, 4), (3, 2, 11), (1, 2, 12)])
@pytest.mark.parametrize("absorb", [False, True])
def test_sumcheck_matches_oracle(field, k, D, n_vars, absorb):
    c = ctx_for(field)
    tabs = [orc.fill_random(field, 500 + 10 * f + k + D, 1 << n_vars) for f in range(k)]
    claimed = sum_elems(field, orc.prod_reduce(field, n_vars, tabs))
    want_rp, want_ch = orc.sumcheck_prove(field, n_vars, tabs, D, claimed, absorb)
    pp = ProductPoly.new([MLE.new(c, n_vars, t) for t in tabs])
    prover = SumcheckProver(D)
    for consume in (False, True):   # consume last: it overwrites the tables
        proof, ch = prover._run(pp, claimed, absorb, consume)
        assert np.array_equal(proof.round_polys, want_rp)
        assert np.array_equal(ch, want_ch)
        if not consume:
            for q, t in zip(pp.polynomials, tabs):
                assert np.array_equal(q.evaluation_slice(), t)   # inputs intact
    if D >= k:
        sub = SumcheckVerifier.verify_partial(field, proof) if not absorb else None
        if sub is not None:
            fresh = ProductPoly.new([MLE.new(c, n_vars, t) for t in tabs])
            assert np.array_equal(fresh.evaluate(sub.challenges), sub.sum)
        else:
            fresh = ProductPoly.new([MLE.new(c, n_vars, t) for t in tabs])
            assert SumcheckVerifier.verify(fresh, proof) is True


def test_sumcheck_zero_variables_and_host_form():
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    pp = ProductPoly.new([MLE.new(c, 0, F(field, [7]))])
    proof, ch = SumcheckProver(2).prove_partial(pp, zk_amd.fe_from_int(field, 7))
    assert proof.round_polys.shape[0] == 0 and ch.shape[0] == 0


# ------------------------------------------------------------------ fft crate vs oracle
@pytest.mark.parametrize("field", FIELDS)
def test_fft_small_vs_faithful_oracle(field):
    c = ctx_for(field)
    for lg in range(0, 9):
        v = orc.fill_random(field, 600 + lg, 1 << lg)
        f = zk_amd.fft(c, v)
        assert np.array_equal(f, orc.fft(field, v))
        assert np.array_equal(zk_amd.ifft(c, f), v)
    w = orc.root_of_unity(field, 16)
    w3 = orc.pow_(field, w, 3)   # fft_internal with a caller-chosen primitive root
    v = orc.fill_random(field, 77, 16)
    got = zk_amd.fft_internal(c, v, w3)
    want = np.zeros_like(v)
    orc._check(orc._lib.orc_fft_internal(field, orc._p(v), orc._c.c_uint64(16), orc._p(w3), orc._p(want)))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("lg", [10, 13, 16])
def test_fft_medium_vs_oracle_fast(field, lg):
    c = ctx_for(field)
    v = orc.fill_random(field, 700 + lg, 1 << lg)
    f = zk_amd.fft(c, v)
    assert np.array_equal(f, orc.ntt_fast(field, v))
    assert np.array_equal(zk_amd.ifft(c, f), v)


@pytest.mark.parametrize("lg", [8, 9, 11, 12, 15, 17, 18, 20])
def test_fft_lds_passes_vs_oracle_fast(lg):
    """sizes that exercise 2 passes (2^8..2^16), 3 passes (2^17..2^24) and uneven radix splits, BN254 + one other field"""
    for field in (zk_amd.BN254_FR, FIELDS[lg % 3]):
        c = ctx_for(field)
        v = orc.fill_random(field, 800 + lg, 1 << lg)
        f = zk_amd.fft(c, v)
        assert np.array_equal(f, orc.ntt_fast(field, v))
        assert np.array_equal(zk_amd.ifft(c, f), v)


@pytest.mark.parametrize("lg", [8, 10, 13])
def test_fft_internal_user_omega_on_the_multipass_plan(lg):
    """fft_internal(values, omega) (fft/src/lib.rs:21-46) with a primitive root other than get_root_of_unity's, at sizes
    that run the LDS multi-pass plan with tables built for that omega; the oracle's faithful recursion is the checker."""
    field = zk_amd.BLS12_377_FR
    c = ctx_for(field)
    n = 1 << lg
    w = orc.pow_(field, orc.root_of_unity(field, n), 5)      # still a primitive n-th root (5 is odd)
    v = orc.fill_random(field, 900 + lg, n)
    want = np.zeros_like(v)
    orc._check(orc._lib.orc_fft_internal(field, orc._p(v), orc._c.c_uint64(n), orc._p(w), orc._p(want)))
    assert np.array_equal(zk_amd.fft_internal(c, v, w), want)


def test_config5_ntt_2_24_properties():
    """config[4]: 2^24-point NTT on one GPU.  (a) ifft(fft(x)) == x on the device-resident vector; (b) two output
    coefficients against the definition X[k] = sum_j x[j] w^(jk): X[0] = sum x[j] and X[n/2] = sum (-1)^j x[j]
    (w^(n/2) = -1), computed exactly with Python integers (Montgomery representatives add like the values)."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    lg = 24
    x = MLE.random(c, lg, 0x5EED0000 + 5, 0)
    X, back = MLE.alloc(c, lg), MLE.alloc(c, lg)
    zk_amd.ntt(c, x, X)
    zk_amd.ntt(c, X, back, inverse=True)
    xs = x.evaluation_slice()
    assert np.array_equal(back.evaluation_slice(), xs)
    Xs = X.evaluation_slice()
    p = zk_amd.modulus(field)

    def exact_col_sum(col):   # exact sum of a uint64 column: 32-bit halves, chunked so uint64 partial sums cannot wrap
        lo = (col & np.uint64(0xFFFFFFFF)).reshape(-1, 1 << 12).sum(axis=1, dtype=np.uint64)
        hi = (col >> np.uint64(32)).reshape(-1, 1 << 12).sum(axis=1, dtype=np.uint64)
        return sum(int(v) for v in lo) + (sum(int(v) for v in hi) << 32)

    def mont_sum(rows):
        return sum(exact_col_sum(np.ascontiguousarray(rows[:, i])) << (64 * i) for i in range(4)) % p

    def limbs_to_int(r):
        return int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192)

    s_even, s_odd = mont_sum(xs[0::2]), mont_sum(xs[1::2])
    assert limbs_to_int(Xs[0]) == (s_even + s_odd) % p
    assert limbs_to_int(Xs[1 << (lg - 1)]) == (s_even - s_odd) % p


def test_fft_error_behaviour():
    c = ctx_for(zk_amd.BN254_FR)
    with pytest.raises(ZkError, match="get_root_of_unity"):      # fft/src/lib.rs:6 unwrap on None
        zk_amd.fft(c, F(zk_amd.BN254_FR, [1, 2, 3]))
    with pytest.raises(ZkError, match="get_root_of_unity"):
        zk_amd.fft(c, np.zeros((0, 4), dtype=np.uint64))
    with pytest.raises(ZkError, match="values must be a power of 2"):   # fft/src/lib.rs:28-30
        zk_amd.fft_internal(c, F(zk_amd.BN254_FR, [1, 2, 3]), zk_amd.fe_from_int(zk_amd.BN254_FR, 5))


# ------------------------------------------------------------------ full-size properties (BASELINE.json configs)
def test_config2_20var_fold_and_sumcheck_properties():
    """config[1]: 20-var MLE fold + full sumcheck on one GPU.  Too large for the faithful oracle in seconds, so:
    (a) the fold is checked against the oracle on the full table (one fold is cheap), (b) the sumcheck proof must
    verify (restated verifier) and its subclaim must equal the product evaluated at the challenges."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    n = 20
    A, B = MLE.random(c, n, 0x5EED0000 + 2, 0), MLE.random(c, n, 0x5EED0000 + 2, 1 << n)
    tabA = A.evaluation_slice()
    r = orc.fill_random(field, 4242, 1)
    assert np.array_equal(A.partial_evaluate(0, r).evaluation_slice(), orc.mle_partial_evaluate(field, n, tabA, 0, r))
    pp = ProductPoly.new([A, B])
    s = pp.round_sums(1)
    claimed = orc.add(field, s[0], s[1])
    assert np.array_equal(claimed, sum_elems(field, orc.prod_reduce(field, n, [tabA, B.evaluation_slice()])))
    proof, ch = SumcheckProver(2).prove_partial(pp, claimed)
    sub = SumcheckVerifier.verify_partial(field, proof)
    assert np.array_equal(sub.challenges, ch)
    assert np.array_equal(pp.evaluate(ch), sub.sum)


def test_config4_gkr_shaped_layers_verify():
    """config[3]: the reference has no gkr crate; its building block is prove_partial / verify_partial on a
    ProductPoly per layer.  Depth 8, width 2^14 here (2^20 in bench.py), 3 factors, degree 3: every layer's proof must
    pass the restated verifier and its subclaim must equal the product evaluated at the challenges."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    n = 14
    for layer in range(8):
        pp = ProductPoly.new([MLE.random(c, n, 0x7000 + 16 * layer + f, 0) for f in range(3)])
        s = pp.round_sums(3)
        claimed = orc.add(field, s[0], s[1])
        proof, ch = SumcheckProver(3).prove_partial(pp, claimed)
        sub = SumcheckVerifier.verify_partial(field, proof)
        assert np.array_equal(sub.challenges, ch)
        assert np.array_equal(pp.evaluate(ch), sub.sum)


def test_25var_prover_beyond_the_capped_grid():
    """2^25-element table: the round kernel needs more than 2048 workgroups to keep <= 16 pairs per thread (lazy
    reduction bound).  k = 1, D = 1: the proof must verify and its subclaim must equal the table evaluated at the
    challenges (size-independent property; the faithful oracle would take minutes here)."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    n = 25
    A = MLE.random(c, n, 0x5EED0000 + 25, 0)
    pp = ProductPoly.new([A])
    s = pp.round_sums(1)
    claimed = orc.add(field, s[0], s[1])
    proof, ch = SumcheckProver(1).prove_partial(pp, claimed)
    sub = SumcheckVerifier.verify_partial(field, proof)
    assert np.array_equal(sub.challenges, ch)
    assert np.array_equal(A.evaluate(ch), sub.sum)
    A.free()


def test_config_24var_fold_properties():
    """metric config: 2^24-element BN254 table.  Size-independent checks: (a) evaluate(T, [r, rest]) ==
    evaluate(fold(T, r), rest); (b) linearity of the fold in r on a strided sample vs the oracle's field ops."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    n = 24
    T = MLE.random(c, n, 0x5EED0000 + 24, 0)
    out = MLE.alloc(c, n - 1)
    pt = orc.fill_random(field, 31337, n)
    T.fold_into(pt[0], out)
    assert np.array_equal(T.evaluate(pt), out.evaluate(pt[1:]))
    # spot-check 64 output elements against the oracle formula on regenerated inputs
    half = 1 << (n - 1)
    got = out.evaluation_slice()
    for j in [0, 1, 63, 64, 12345, half // 2, half - 1] + [random.Random(1).randrange(half) for _ in range(57)]:
        lo = orc.fill_random(field, 0x5EED0000 + 24, 1, first_index=j)[0]
        hi = orc.fill_random(field, 0x5EED0000 + 24, 1, first_index=j + half)[0]
        want = orc.sub(field, lo, orc.mul(field, pt[0], orc.sub(field, lo, hi)))
        assert np.array_equal(got[j], want)


_EVAL_CHILD = """
import sys, numpy as np
sys.path.insert(0, %r)
import zk_amd
from oracle import binding as orc
for field in (zk_amd.BN254_FR, zk_amd.BLS12_381_FR):
    c = zk_amd.Context(field, 0)
    for n in (1, 8, 9, 12, 13, 17, 20):
        tab = orc.fill_random(field, 4100 + n, 1 << n)
        pt = orc.fill_random(field, 4200 + n, n)
        assert np.array_equal(zk_amd.MultiLinearPolynomial.new(c, n, tab).evaluate(pt), orc.mle_evaluate(field, n, tab, pt)), (field, n)
print("evaluate ok")
"""


@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_every_arity(field):
    """evaluate (evaluation_form.rs:83-89) at every arity 1..21 (BN254: ..23): above 2^20 elements the top 1-4 variables go first
    (k_fold_eq), then the bulk kernel takes the low 8-12 variables per launch (k_eval_low), the one-workgroup tail the rest; edge
    points (0, 1, p - 1 coordinates) included.  Bit-exact vs the oracle."""
    c = ctx_for(field)
    p = zk_amd.modulus(field)
    for n in range(1, 24 if field == zk_amd.BN254_FR else 22):
        tab = orc.fill_random(field, 4000 + n, 1 << n)
        t = MLE.new(c, n, tab)
        pts = [orc.fill_random(field, 4300 + n, n)]
        if n in (9, 10, 13, 20, 22):
            edge = [0, 1, p - 1, 2]
            pts.append(F(field, [edge[(i * 7 + n) % 4] for i in range(n)]))
        for pt in pts:
            assert np.array_equal(t.evaluate(pt), orc.mle_evaluate(field, n, tab, pt)), n
        t.free()


def test_evaluate_fold_path_still_exact():
    """ZK_EVAL_FOLDS=1 keeps the variable-by-variable evaluate (k_fold_multi + tail) for A/B runs: same results."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _EVAL_CHILD % root], env=dict(os.environ, ZK_EVAL_FOLDS="1"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "evaluate ok" in r.stdout, r.stdout + r.stderr


_EVAL_STREAM_CHILD = """
import os, sys, numpy as np
sys.path.insert(0, %r)
import zk_amd
from oracle import binding as orc
checked = 0
SIZES = tuple(int(x) for x in os.environ.get("ZK_EVAL_SIZES", "19,20,21,22").split(","))
ALL_FIELDS = os.environ.get("ZK_EVAL_ALL_FIELDS") == "1"
MAXN = int(os.environ.get("ZK_EVAL_MAXN", "19"))
for field in (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR):
    c = zk_amd.Context(field, 0)
    p = zk_amd.modulus(field)
    for n in SIZES:          # ZK_EVAL_STREAM_MIN=19: k_eval_stream with L = 10, 11, 12, 13 at n = 19..22 (9 variables left)
        if n > 20 and field != zk_amd.BN254_FR and not ALL_FIELDS:
            continue
        tab = orc.fill_random(field, 4500 + n, 1 << n)
        t = zk_amd.MultiLinearPolynomial.new(c, n, tab)
        pts = [orc.fill_random(field, 4600 + n, n)]
        edge = [0, 1, p - 1, 2]
        pts.append(orc.from_ints(field, [edge[(i * 7 + n) %% 4] for i in range(n)]))
        for pt in pts:
            assert np.array_equal(t.evaluate(pt), orc.mle_evaluate(field, n, tab, pt)), (field, n)
            checked += 1
        t.free()
    # worst case of the column sums: every element p - 1 (all limbs of the halves near their maxima) at a point of p - 1's
    n = MAXN
    tab = np.tile(orc.from_int(field, p - 1), (1 << n, 1))
    pt = orc.from_ints(field, [p - 1 - i for i in range(n)])
    t = zk_amd.MultiLinearPolynomial.new(c, n, tab)
    assert np.array_equal(t.evaluate(pt), orc.mle_evaluate(field, n, tab, pt)), (field, "max")
    t.free()
    checked += 1
print("evaluate stream ok", checked)
"""


def test_evaluate_streaming_kernel_forced_at_small_sizes():
    """k_eval_stream (eval_kernels.cuh: half an element per lane, carry-free 29-bit column sums, up to 15 low variables per
    launch) normally starts at 21 variables; a child process with ZK_EVAL_STREAM_MIN=19 puts n = 19..22 (L = 10..13) through it on
    all three fields, random and edge points plus the all-(p - 1) table, bit-exact vs the oracle (evaluation_form.rs:83-89)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # 9 variables left (512 workgroups: L = 10, 11, 12, 13) and the shipped choice (8 left up to 21 variables: L = 11, 12, 13, 13)
    # ... and 7 variables left at n = 21, 22: L = 14 (128 rows per lane) and L = 15 (256 rows: the redc bound 2^136 * p of the column
    # sums) on ALL three fields, the all-(p - 1) table at L = 15 (L = 14 was never run, L >= 13 only on BN254)
    for extra in (dict(ZK_EVAL_STREAM_LEAVE="9"), dict(),
                  dict(ZK_EVAL_STREAM_LEAVE="7", ZK_EVAL_SIZES="21,22", ZK_EVAL_ALL_FIELDS="1", ZK_EVAL_MAXN="22")):
        env = {k: v for k, v in os.environ.items() if k not in ("ZK_EVAL_STREAM_LEAVE", "ZK_EVAL_SIZES", "ZK_EVAL_ALL_FIELDS", "ZK_EVAL_MAXN")}
        r = subprocess.run([sys.executable, "-c", _EVAL_STREAM_CHILD % root], env=dict(env, ZK_EVAL_STREAM_MIN="19", **extra),
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "evaluate stream ok" in r.stdout, str(extra) + r.stdout + r.stderr


def test_evaluate_unweighted_second_stage_still_exact():
    """ZK_EVAL_WEIGHT=0 switches off the eq(point_high, g) weights of the bulk launches (the shape tables of more than 27 variables
    take, where more than 12 variables are left after a launch): the second stage is then a bulk launch of its own, as in round 3.
    Same results, through k_eval_low (n <= 20) and k_eval_stream (n = 21)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = _EVAL_CHILD.replace("(1, 8, 9, 12, 13, 17, 20)", "(1, 8, 9, 12, 13, 17, 20, 21)")
    r = subprocess.run([sys.executable, "-c", child % root], env=dict(os.environ, ZK_EVAL_WEIGHT="0"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "evaluate ok" in r.stdout, r.stdout + r.stderr


def test_evaluate_n24_vs_oracle():
    """The reference's own benchmark operation at the metric's table size: evaluate on 2^24 BN254-Fr elements (k_eval_stream with
    L = 15, then one k_eval_low workgroup) against the oracle's n folds, at a random point and at a point with 0 / 1 / p - 1
    coordinates (the r = 0 / r = 1 shortcuts of evaluation_form.rs:61-62)."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    n = 24
    p = zk_amd.modulus(field)
    tab = orc.fill_random(field, 0x5EED0000 + 24, 1 << n)
    t = MLE.new(c, n, tab)
    edge = [0, 1, p - 1, 2]
    for pt in (orc.fill_random(field, 4724, n), F(field, [edge[(i * 5 + 1) % 4] for i in range(n)])):
        assert np.array_equal(t.evaluate(pt), orc.mle_evaluate(field, n, tab, pt))
    t.free()


# Forced kernel-selection paths (the library reads its ZK_* switches once per process: each switch set is a child process running
# tests/skip1_check.py over the (k, D) grid, wrong claimed sums and the two-term GKR layer shape, every proof compared with the oracle
# bit for bit).  The children are independent: they run four at a time (the box admits six processes on its card), and the oracle
# proofs of the whole grid are computed once, before them, on CPU-only workers (tests/oracle_cache.py) instead of in every child.
SKIP1_RUNS = {
    # SKIP1 kernels everywhere (no quad kernel, no pipeline: they would take the small rounds)
    "skip1_everywhere": dict(ZK_SKIP1_MIN_PAIRS="1", ZK_QUAD_MAX_PAIRS="0", ZK_PIPE_MAX_PAIRS="0"),
    # plain k_round_kd at small sizes
    "plain_kd_small": dict(ZK_QUAD_MAX_PAIRS="0", ZK_PIPE_MAX_PAIRS="0"),
    # the four-lanes-per-pair kernel + classic tails (the pipeline off)
    "quad_classic_tails": dict(ZK_PIPE_MAX_PAIRS="0", ZK_CHECK_SIZES="7,11,13,15"),
    # the pipeline from 2^17 pairs down, entered right after SKIP1 rounds (the transcript block derives S(1))
    "pipe_from_2p17_after_skip1": dict(ZK_PIPE_MAX_PAIRS="131072", ZK_SKIP1_MIN_PAIRS="1", ZK_CHECK_SIZES="11,12,13,15,17"),
    # the pipeline with defaults at more sizes
    "pipe_defaults": dict(ZK_CHECK_SIZES="10,12,14,16,18"),
    # LEAD kernels everywhere (slot D = leading coefficient, the tail rebuilds S(D)): with SKIP1 in every fused round, classic tails
    "lead_skip1_classic": dict(ZK_LEAD_MIN_PAIRS="1", ZK_SKIP1_MIN_PAIRS="1", ZK_QUAD_MAX_PAIRS="0", ZK_PIPE_MAX_PAIRS="0"),
    # ... and with the pipeline entered right after a LEAD + SKIP1 round (the transcript block derives S(1), then rebuilds S(D))
    "lead_skip1_pipe": dict(ZK_LEAD_MIN_PAIRS="1", ZK_SKIP1_MIN_PAIRS="1", ZK_QUAD_MAX_PAIRS="0", ZK_CHECK_SIZES="11,12,13,15"),
    # LEAD in round 0 only (sums-only kernel), everything else default
    "lead_round0": dict(ZK_LEAD_MIN_PAIRS="1", ZK_CHECK_SIZES="3,9,14,16"),
    # round 0 on the wide-accumulator kernel (k_round_kd<2,2,sums only,LEAD>: the A/B fallback of k_round0_dot29) ...
    "round0_wide": dict(ZK_ROUND0_DOT29="0", ZK_LEAD_MIN_PAIRS="1", ZK_CHECK_SIZES="3,9,14"),
    # ... and the carry-free round-0 kernel for the product-plus-term shape as well (k_round0_dot29<1>, not selected by default)
    "round0_dot29_terms": dict(ZK_ROUND0_DOT29="2", ZK_LEAD_MIN_PAIRS="1", ZK_CHECK_SIZES="3,9,13,14"),
    # SKIP1 + LEAD everywhere with the claim evaluated by the TAILS (round 4's form; shipped: the round kernel's claim workgroup), with
    # and without the pipeline behind them (k_round_tail / the deferred tail of the first pipelined launch)
    # the LDS-DMA round kernels (k_round0_glds, k_round_fused_glds<2 / 3>; cached half tables below 256 pairs, nontemporal above) wherever
    # a round has a multiple of 64 pairs: classic tails behind them, then the pipeline entered right after them, then the three-table
    # shape and the batched twins on bigger tables; and OFF at sizes where the defaults select them (the kernels they replaced)
    "glds_classic_tails": dict(ZK_ROUND_GLDS_MIN_PAIRS="64", ZK_ROUND_GLDS_NT_MIN_PAIRS="256", ZK_LEAD_MIN_PAIRS="1", ZK_SKIP1_MIN_PAIRS="1",
                               ZK_QUAD_MAX_PAIRS="0", ZK_PIPE_MAX_PAIRS="0", ZK_CHECK_SIZES="7,8,9,11,13,15"),
    "glds_then_pipe": dict(ZK_ROUND_GLDS_MIN_PAIRS="64", ZK_ROUND_GLDS_NT_MIN_PAIRS="256", ZK_LEAD_MIN_PAIRS="1", ZK_SKIP1_MIN_PAIRS="1",
                           ZK_QUAD_MAX_PAIRS="0", ZK_CHECK_SIZES="11,12,13,15"),
    "glds_defaults_n18_to_20": dict(ZK_CHECK_SIZES="18,19,20", ZK_CHECK_FIELDS="2"),
    # the shipped thresholds where round 0 of two tables (2^21 pairs) and the product-plus-term kernels (2^20 / 2^19) reach them
    "glds_defaults_n21_22": dict(ZK_CHECK_SIZES="21,22", ZK_CHECK_FIELDS="1"),
    "glds_off_n19_20": dict(ZK_ROUND_GLDS="0", ZK_CHECK_SIZES="19,20", ZK_CHECK_FIELDS="1"),
    # the initial sponge stored by a launch of its own in front of round 0 (until round 6; shipped: an argument of round 0's tail)
    "sponge_by_its_own_launch": dict(ZK_SPONGE_IN_TAIL="0", ZK_CHECK_SIZES="2,9,13,14,17", ZK_CHECK_FIELDS="2"),
    "claim_in_tails": dict(ZK_CLAIM_IN_ROUND="0", ZK_LEAD_MIN_PAIRS="1", ZK_SKIP1_MIN_PAIRS="1", ZK_QUAD_MAX_PAIRS="0", ZK_CHECK_SIZES="3,7,11,13",
                           ZK_CHECK_FIELDS="2"),
}
_SWEEP_ENV_KEYS = ("ZK_SKIP1_MIN_PAIRS", "ZK_QUAD_MAX_PAIRS", "ZK_PIPE_MAX_PAIRS", "ZK_CHECK_SIZES", "ZK_LEAD_MIN_PAIRS", "ZK_ROUND0_DOT29",
                   "ZK_CHECK_FIELDS", "ZK_CLAIM_IN_ROUND", "ZK_ROUND_GLDS", "ZK_ROUND_GLDS_MIN_PAIRS", "ZK_ROUND_GLDS_NT_MIN_PAIRS",
                   "ZK_SPONGE_IN_TAIL")


@pytest.fixture(scope="module")
def skip1_sweeps(tmp_path_factory):
    """prefill the oracle cache for the union of the runs' grids, then start every child (four at a time); -> {name: Future}"""
    from concurrent.futures import ThreadPoolExecutor

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_cache
    import skip1_check

    cache = str(tmp_path_factory.mktemp("oracle_cache"))
    base = {k: v for k, v in os.environ.items() if k not in _SWEEP_ENV_KEYS}
    base["ZK_ORACLE_CACHE"] = cache
    spec = []
    for extra in SKIP1_RUNS.values():
        sizes = tuple(int(x) for x in extra.get("ZK_CHECK_SIZES", "2,3,7,11,13").split(","))
        spec += skip1_check.spec(sizes, int(extra.get("ZK_CHECK_FIELDS", "3")))
    os.environ["ZK_ORACLE_CACHE"] = cache
    try:
        oracle_cache.prefill(spec, workers=min(12, max(2, (os.cpu_count() or 4) - 2)))
    finally:
        del os.environ["ZK_ORACLE_CACHE"]

    def child(extra):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "skip1_check.py")], env=dict(base, **extra), capture_output=True,
                              text=True, timeout=900)

    pool = ThreadPoolExecutor(max_workers=4)
    futures = {name: pool.submit(child, extra) for name, extra in SKIP1_RUNS.items()}
    yield futures
    pool.shutdown(wait=True)


@pytest.mark.parametrize("name", list(SKIP1_RUNS))
def test_skip1_rounds_bit_exact(skip1_sweeps, name):
    """Big fused rounds leave out the t = 1 sums and derive S(1) from the previous round's claim (k_round_kd SKIP1, TailDerive), LEAD
    rounds rebuild S(D), pipelined rounds interpolate: one child process per switch set proves the grid that way and compares every
    proof with the oracle bit for bit (tests/skip1_check.py).  A failure names its switch set."""
    r = skip1_sweeps[name].result()
    assert r.returncode == 0 and "skip1 ok" in r.stdout, str(SKIP1_RUNS[name]) + r.stdout + r.stderr


def test_beyond_baseline_sizes_properties():
    """Sizes past BASELINE.json's (byte offsets beyond 2^32, 288 GB HBM): a 26-variable sumcheck verified end to end, a
    27-variable fold and a 2^25-point NTT round trip, each checked through a size-independent property (tables are
    compared by their MLE value at a random point instead of being downloaded)."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    p = zk_amd.modulus(field)
    rng = random.Random(2627)
    # sumcheck n = 26: verify_partial accepts and the sub-claim equals the product at the challenge point (verifier.rs:27-31)
    n = 26
    A, B = MLE.random(c, n, 2601, 0), MLE.random(c, n, 2602, 0)
    pp = ProductPoly.new([A, B])
    s = pp.round_sums(1)
    claimed = zk_amd.fe_from_int(field, (zk_amd.fe_to_int(field, s[0]) + zk_amd.fe_to_int(field, s[1])) % p)
    proof, ch = SumcheckProver(2).prove_partial(pp, claimed)
    sub = SumcheckVerifier.verify_partial(field, proof)
    assert np.array_equal(sub.challenges, ch)
    assert zk_amd.fe_to_int(field, pp.evaluate(ch)) == zk_amd.fe_to_int(field, sub.sum)
    A.free(); B.free()
    # fold n = 27 at r: evaluating the folded table at z equals evaluating the original at (r, z)  (evaluation_form.rs:83-89)
    m = 27
    T = MLE.random(c, m, 2701, 0)
    r = rng.randrange(p)
    z = [rng.randrange(p) for _ in range(m - 1)]
    folded = T.partial_evaluate(0, F(field, [r]))
    assert zk_amd.fe_to_int(field, folded.evaluate(F(field, z))) == zk_amd.fe_to_int(field, T.evaluate(F(field, [r] + z)))
    T.free(); folded.free()
    # NTT 2^25: ifft(fft(x)) == x  (fft/src/lib.rs:78-82), compared at a random MLE point
    k = 25
    x, y, w = MLE.random(c, k, 2501, 0), MLE.alloc(c, k), MLE.alloc(c, k)
    zk_amd.ntt(c, x, y, False)
    zk_amd.ntt(c, y, w, True)
    pt = F(field, [rng.randrange(p) for _ in range(k)])
    assert zk_amd.fe_to_int(field, w.evaluate(pt)) == zk_amd.fe_to_int(field, x.evaluate(pt))
    assert zk_amd.fe_to_int(field, y.evaluate(pt)) != zk_amd.fe_to_int(field, x.evaluate(pt))
    x.free(); y.free(); w.free()


# ---- round 2 additions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_partial_eq_on_device(field):
    """#[derive(PartialEq)] (evaluation_form.rs:4) through zk_mle_equal"""
    c = zk_amd.Context(field, 0)
    t = orc.fill_random(field, 31, 1 << 11)
    a, b = MLE.new(c, 11, t), MLE.new(c, 11, t)
    assert a == b and a == a.clone()
    t2 = t.copy()
    t2[-1, 3] ^= np.uint64(1)   # one bit in the last limb of the last element
    assert a != MLE.new(c, 11, t2)
    assert a != MLE.new(c, 10, t[: 1 << 10])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k,D,n_vars", [(2, 2, 6), (2, 4, 7), (4, 4, 6), (3, 3, 9), (2, 2, 13)])
def test_product_with_a_repeated_factor(field, k, D, n_vars):
    """ProductPoly::new(vec![a.clone(), a, ..]) is legal in the reference (it owns clones); the same HANDLE listed twice
    must give the same proof, also with consume (in-place folds would fold the shared buffer once per listing)."""
    c = zk_amd.Context(field, 0)
    t = orc.fill_random(field, 41, 1 << n_vars)
    u = orc.fill_random(field, 42, 1 << n_vars)
    tabs = [t, t] + [u] * (k - 2)
    claimed = orc.sum_elems(field, orc.prod_reduce(field, n_vars, tabs))   # iter().sum::<F>()
    want_rp, want_ch = orc.sumcheck_prove(field, n_vars, tabs, D, claimed, False)
    for consume in (False, True):
        a, b = MLE.new(c, n_vars, t), MLE.new(c, n_vars, u)
        pp = ProductPoly.new([a, a] + [b] * (k - 2))
        proof, ch = zk_amd.SumcheckProver(D)._run(pp, claimed, False, consume)
        assert np.array_equal(proof.round_polys, want_rp) and np.array_equal(ch, want_ch), consume


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("lg", [1, 2, 4, 6, 9])
def test_fft_internal_with_a_non_primitive_omega(field, lg):
    """fft_internal(values, omega) takes ANY omega (fft/src/lib.rs:21): the reference multiplies by omega^(i + n/2)
    literally (:41), which is -omega^i only for a primitive n-th root.  Random omega, omega = 1, and a primitive root of
    the wrong order, against the faithful recursive oracle."""
    c = zk_amd.Context(field, 0)
    n = 1 << lg
    v = orc.fill_random(field, 51 + lg, n)
    omegas = [orc.fill_random(field, 52, 1)[0], zk_amd.fe_from_int(field, 1), zk_amd.root_of_unity(field, lg + 2)]
    for w in omegas:
        want = np.zeros_like(v)
        orc._check(orc._lib.orc_fft_internal(field, orc._p(v), orc._c.c_uint64(n), orc._p(w), orc._p(want)))
        assert np.array_equal(zk_amd.fft_internal(c, v, w), want)


def test_sample_n_and_trim():
    field = zk_amd.BN254_FR
    t1, t2 = zk_amd.Transcript(), zk_amd.Transcript()
    t1.append(b"abc")
    t2.append(b"abc")
    many = t1.sample_n_field_elements(field, 5)                      # zk_transcript_sample_n_field_elements
    assert np.array_equal(many, np.stack([t2.sample_field_element(field) for _ in range(5)]))
    assert t1.sample_n_field_elements(field, 0).shape == (0, 4)
    c = zk_amd.Context(field, 0)
    a = MLE.random(c, 20, 1, 0)
    want = a.evaluation_slice()
    b = a.clone()
    b.free()
    c.trim()                                                         # zk_ctx_trim: the freed block goes back to the device
    assert np.array_equal(a.evaluation_slice(), want)


# ------------------------------------------------------------------ BASELINE configs at their OWN sizes, bit-exact vs the oracle
def _prove_vs_oracle(field, n, k, D, seed):
    c = ctx_for(field)
    polys = [MLE.random(c, n, seed, f << n) for f in range(k)]
    tabs = [q.evaluation_slice() for q in polys]
    for f, t in enumerate(tabs):   # the device generator is the oracle's generator: pin it on a slice
        assert np.array_equal(t[:4096], orc.fill_random(field, seed, 4096, first_index=f << n))
    pp = ProductPoly.new(polys)
    s = pp.round_sums(1)
    claimed = orc.add(field, s[0], s[1])
    want_rp, want_ch = orc.sumcheck_prove(field, n, tabs, D, claimed, False)   # the faithful restatement (prover.rs:33-73)
    proof, ch = SumcheckProver(D).prove_partial(pp, claimed)                    # default kernel thresholds
    assert np.array_equal(proof.round_polys, want_rp), "round polynomials differ from the oracle"
    assert np.array_equal(ch, want_ch), "challenges differ from the oracle"
    sub = SumcheckVerifier.verify_partial(field, proof)                        # and the claimed sum was the true one
    assert np.array_equal(sub.challenges, ch)
    assert np.array_equal(pp.evaluate(ch), sub.sum)
    for q in polys:
        q.free()


@pytest.mark.parametrize("k,D", [(2, 2), (3, 3)])
def test_config2_n20_prover_bit_exact_at_default_thresholds(k, D):
    """BASELINE config[1] ("20-var MLE fold + full sumcheck on 1xMI355X, bit-exact vs CPU"): the whole proof -- every round
    polynomial and challenge -- equal to the faithful oracle's, with the kernel thresholds the product ships (SKIP1 rounds from
    2^16 pairs, quad rounds, pipelined rounds, finisher: every path at its real size).  prover.rs:44-68."""
    _prove_vs_oracle(zk_amd.BN254_FR, 20, k, D, 0x5EED0000 + 20)


def test_config3_n24_prover_and_fold_bit_exact():
    """The metric's own size: n = 24, k = 2, D = 2 proof equal to the faithful oracle's (round 0 on 2 x 512 MiB, SKIP1 fused
    rounds at 2^22..2^16 pairs), and the timed fold (partial_evaluate(0, [r]) of the 2^24 table, evaluation_form.rs:40-80)
    equal to the oracle's on ALL 2^23 outputs."""
    field = zk_amd.BN254_FR
    _prove_vs_oracle(field, 24, 2, 2, 0x5EED0000 + 24)
    c = ctx_for(field)
    T = MLE.random(c, 24, 0x5EED0000 + 24, 0)
    out = MLE.alloc(c, 23)
    r = orc.fill_random(field, 0xC4A11, 1)
    T.fold_into(r[0], out)
    want = orc.mle_partial_evaluate(field, 24, T.evaluation_slice(), 0, r)
    assert np.array_equal(out.evaluation_slice(), want)
    T.free(); out.free()


def test_config5_ntt_2_24_outputs_vs_the_definition():
    """config[4]: sixteen random outputs (+ the corners) of the 2^24-point forward and inverse transforms against the
    definition X[k] = sum_j x[j] w^(jk) evaluated by the oracle (orc_dft_point, fft/src/lib.rs:39-45): the 8+8+8 pass plan
    exists only at this size, and a forward/inverse-symmetric addressing error would survive the round trip."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    lg = 24
    x = MLE.random(c, lg, 0x5EED0000 + 5, 0)
    X, Y = MLE.alloc(c, lg), MLE.alloc(c, lg)
    zk_amd.ntt(c, x, X)
    zk_amd.ntt(c, x, Y, inverse=True)
    xs, Xs, Ys = x.evaluation_slice(), X.evaluation_slice(), Y.evaluation_slice()
    rng = random.Random(0x2424)
    ks = [0, 1, (1 << lg) - 1, 1 << 8, 1 << 16, (1 << 23) + 1] + [rng.randrange(1 << lg) for _ in range(16)]
    for k in ks:
        assert np.array_equal(Xs[k], orc.dft_point(field, xs, k)), f"forward output {k}"
    for k in ks[:3] + ks[6:12]:
        assert np.array_equal(Ys[k], orc.dft_point(field, xs, k, inverse=True)), f"inverse output {k}"
    x.free(); X.free(); Y.free()


@pytest.mark.parametrize("lg", [21, 22])
def test_ntt_full_compare_at_2_21_and_2_22(lg):
    """every output of the 3-pass plan at 2^21 (7+7+7) / 2^22 against the oracle's iterative transform (itself checked against
    the faithful recursion at small sizes)"""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    x = MLE.random(c, lg, 0x5EED0000 + lg, 0)
    X, B = MLE.alloc(c, lg), MLE.alloc(c, lg)
    zk_amd.ntt(c, x, X)
    xs = x.evaluation_slice()
    assert np.array_equal(X.evaluation_slice(), orc.ntt_fast(field, xs))
    zk_amd.ntt(c, X, B, inverse=True)
    assert np.array_equal(B.evaluation_slice(), xs)
    x.free(); X.free(); B.free()


def test_verify_with_per_round_lengths_on_the_device_path():
    """zk_sumcheck_verify_lengths (verifier.rs:15-33 with each round interpolated at its own length, :55-58): an honest D = 2
    proof re-stated with extra evaluations of the same round polynomials in some rounds still verifies only if the transcript
    matches -- so the ragged proof is produced round by round with the oracle's transcript -- and equals the oracle's verdict."""
    for field in FIELDS:
        c = ctx_for(field)
        n, k = 6, 2
        tabs = [orc.fill_random(field, 8800 + f, 1 << n) for f in range(k)]
        lens = [3, 4, 3, 5, 3, 4]
        claimed = sum_elems(field, orc.prod_reduce(field, n, tabs))
        tr = orc.Transcript()
        tr.append(b"".join(orc.mle_to_bytes(field, n, t) for t in tabs))
        tr.append(orc.to_bytes_be(field, claimed))
        cur, rounds = [t.copy() for t in tabs], []
        for r in range(n):
            m = n - r
            ys = []
            for t in range(lens[r]):
                parts = [orc.mle_partial_evaluate(field, m, q, 0, orc.from_int(field, t).reshape(1, 4)) for q in cur]
                ys.append(sum_elems(field, orc.prod_reduce(field, m - 1, parts)))
            ys = np.stack(ys)
            rounds.append(ys)
            tr.append(b"".join(orc.to_bytes_be(field, y) for y in ys))
            ch = tr.sample_field_element(field)
            cur = [orc.mle_partial_evaluate(field, m, q, 0, ch.reshape(1, 4)) for q in cur]
        pp = ProductPoly.new([MLE.new(c, n, t) for t in tabs])
        assert orc.sumcheck_verify_lengths(field, n, tabs, claimed, rounds) is True
        assert SumcheckVerifier.verify(pp, SumcheckProof(claimed, rounds)) is True
        rounds[3][4] = orc.add(field, rounds[3][4], orc.from_int(field, 1))   # the extra evaluation is part of the polynomial
        try:
            want = orc.sumcheck_verify_lengths(field, n, tabs, claimed, rounds)
        except orc.OracleError:
            want = "err"
        try:
            got = SumcheckVerifier.verify(pp, SumcheckProof(claimed, rounds))
        except ZkError:
            got = "err"
        assert got == want and got is not True
        with pytest.raises(ZkError, match="require 1 round poly"):
            SumcheckVerifier.verify(pp, SumcheckProof(claimed, rounds[:-1]))


def test_round_sums_through_the_lead_kernels_at_their_real_size():
    """zk_round_sums (prover.rs:49-56 for one round) at 2^18 pairs, where the (2,2) and (3,3) sums-only kernels accumulate the
    leading coefficient and the tail rebuilds S(D) (k_round_kd LEAD): all D + 1 sums equal to the oracle's
    fold -> prod_reduce -> sum, and the round-0 identity S(0) + S(1) = sum of the product table."""
    field = zk_amd.BN254_FR
    c = ctx_for(field)
    n = 19
    for k, D in ((2, 2), (3, 3)):
        polys = [MLE.random(c, n, 0x1EAD + k, f << n) for f in range(k)]
        tabs = [q.evaluation_slice() for q in polys]
        got = ProductPoly.new(polys).round_sums(D)
        want = oracle_round_sums(field, n, tabs, D)
        assert np.array_equal(got, want), (k, D)
        for q in polys:
            q.free()
