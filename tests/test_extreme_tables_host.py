"""Pins tests/extreme_tables.py on the CPU: the builders and their closed forms against the C oracle and against oracle/pyref.py, and the
numbers that are the reason these tables exist.

The round and evaluate kernels bound their unreduced sums over the STORED limbs.  The two older "worst case" tests filled tables with
the VALUE p - 1, whose stored limbs are p - (R mod p): 0.71 p, 0.79 p and 0.29 p for BN254, BLS12-381 and BLS12-377.  At those limbs
kMaxLazy = 32 products reach a wide top word of 0, 4 and 0; the true maxima, at the representation M = p - 1, are 1, 6 and 0
(test_top_words_of_the_wide_accumulator asserts every one of these figures).  No GPU needed."""
import numpy as np
import pytest

import extreme_tables as et
import field_corpus as fc
from oracle import binding as orc
from oracle import pyref

FIELDS = (0, 1, 2)
FIELD_IDS = ["bn254", "bls12_381", "bls12_377"]
CLOSED = [f for f in et.FAMILIES if f != "mixed"] + ["stripe(O,Z)", "const(Z)", "const(ONE)"]


def _family(field, name, n, k):
    if name in et.FAMILIES:
        return et.family(field, name, n, k, fill_random=orc.fill_random, seed=77)
    kind, a, b = et._TWO_RAW[name]
    r = et.raws(field)
    return [et.table(field, name, n)] * k, et.Closed(field, n, kind, [(et.value(field, r[a]), et.value(field, r[b]))] * k)


def test_top_words_of_the_wide_accumulator():
    tops_m, tops_v, ratios = [], [], []
    for field in FIELDS:
        p = fc.MODULI[field]
        r = et.raws(field)
        stored = et.rep(field, p - 1)                 # what a table of the value p - 1 holds
        assert stored == p - r["ONE"] and np.array_equal(orc.from_int(field, p - 1), et.limbs(stored))
        assert et.value(field, r["ONE"]) == 1 and et.value(field, stored) == p - 1
        tops_m.append(et.top_word(field, r["M"]))
        tops_v.append(et.top_word(field, stored))
        ratios.append(round(stored / p, 2))
        assert tops_m[-1] == fc.FieldModel(field).top_max == (fc.K_MAX_LAZY * (p - 1) ** 2) >> 512
    print("top word of 32 M^2:", tops_m, " of 32 rep(p-1)^2:", tops_v, " rep(p-1) / p:", ratios)
    assert tops_m == [1, 6, 0]
    assert tops_v == [0, 4, 0]
    assert ratios == [0.71, 0.79, 0.29]


@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_all_ones_representation(field):
    p = fc.MODULI[field]
    b = p.bit_length()
    r = et.raws(field)
    o = r["O"]
    assert o < p <= 2 * o + 1 and r["O1"] == o - 1 and r["M"] == p - 1 and r["Z"] == 0
    l29 = fc.split29(o)
    assert l29[:8] == [(1 << 29) - 1] * 8
    assert l29[8] == (1 << (b - 1 - 232)) - 1        # every bit below p's top bit
    assert 2 * l29[8] + 1 >= fc.split29(p - 1)[8]    # no canonical value has a top limb beyond one more bit
    assert o & ((1 << 128) - 1) == (1 << 128) - 1 and o >> 128 == (1 << (b - 129)) - 1   # the halves k_eval_stream splits
    assert np.array_equal(et.limbs(o), np.array([2**64 - 1] * 3 + [(1 << (b - 193)) - 1], dtype=np.uint64))


@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_builders_lay_the_halves_as_the_fold_pairs_them(field, n):
    """step: partial_evaluate(0, [0]) gives all a and [1] all b; stripe: the same at the LAST variable"""
    r = et.raws(field)
    a, b = r["M"], r["O"]
    for tab, var in ((et.step_table(a, b, n), 0), (et.stripe_table(a, b, n), n - 1)):
        assert tab.shape == (1 << n, 4) and tab.dtype == np.uint64
        for c, want in ((0, a), (1, b)):
            got = orc.mle_partial_evaluate(field, n, tab, var, orc.from_int(field, c)[None, :])
            assert np.array_equal(got, et.const_table(want, n - 1)), (var, c)
    assert np.array_equal(et.const_table(a, n), np.tile(et.limbs(a), (1 << n, 1)))
    tabs, closed = et.family(field, "mixed", n, 3, fill_random=orc.fill_random, seed=5)
    assert closed is None and np.array_equal(tabs[0], et.const_table(b, n))
    assert np.array_equal(tabs[1], orc.fill_random(field, 6, 1 << n)) and np.array_equal(tabs[2], orc.fill_random(field, 7, 1 << n))
    tabs, closed = et.family(field, "with_zero_factor", n, 3)
    assert not tabs[2].any() and np.array_equal(tabs[0], et.const_table(a, n)) and closed.true_sum() == 0


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_closed_forms_equal_the_c_oracle(field, n, k):
    p = fc.MODULI[field]
    E = lambda vals: et.elems(field, vals)   # noqa: E731
    for name in CLOSED:
        tabs, closed = _family(field, name, n, k)
        for D in (k, k + 1):
            # one round: fold at t, multiply, sum (prover.rs:49-56)
            sums = []
            for t in range(D + 1):
                a = orc.from_int(field, t)[None, :]
                sums.append(orc.sum_elems(field, orc.prod_reduce(field, n - 1, [orc.mle_partial_evaluate(field, n, tb, 0, a) for tb in tabs])))
            assert np.array_equal(np.stack(sums), E(closed.round_sums(D))), (name, D)
            if name == "with_zero_factor":
                assert not np.stack(sums).any()
            # whole proofs, true and wrong claim
            s = closed.true_sum()
            assert np.array_equal(orc.sum_elems(field, orc.prod_reduce(field, n, tabs)), E([s])[0]), name
            for claimed in (s, (s + 5) % p):
                rp, ch = orc.sumcheck_prove(field, n, tabs, D, E([claimed])[0], False)
                crp, cch = closed.prove(D, claimed)
                assert np.array_equal(rp, np.stack([E(r) for r in crp])) and np.array_equal(ch, E(cch)), (name, D)
                assert crp == closed.round_polys(D, cch)
        # evaluation: a random point, all zeros, all ones, and coordinates of representation M and O
        r = et.raws(field)
        for pt in (orc.to_ints(field, orc.fill_random(field, 31 + n, n)), [0] * n, [1] * n,
                   [et.value(field, r["M" if i % 2 else "O"]) for i in range(n)]):
            assert np.array_equal(orc.product_evaluate(field, n, tabs, E(pt)), E([closed.evaluate(pt)])[0]), (name, pt)
            assert np.array_equal(orc.mle_evaluate(field, n, tabs[0], E(pt)), E([closed.factor(0).evaluate(pt)])[0]), (name, pt)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_closed_forms_equal_pyref(field, n, k):
    for name in CLOSED:
        tabs, closed = _family(field, name, n, k)
        poly = pyref.Product([pyref.MLE(field, n, [pyref.from_mont_limbs(field, row) for row in t]) for t in tabs])
        s = closed.true_sum()
        assert sum(poly.prod_reduce()) % fc.MODULI[field] == s
        for claimed in (s, s + 5):
            assert tuple(pyref.sumcheck_prove(poly, claimed, k, False)) == closed.prove(k, claimed), name
        sub, ch = pyref.sumcheck_verify_partial(field, s, closed.prove(k, s)[0])
        assert ch == closed.prove(k, s)[1] and sub == poly.evaluate(ch) == closed.evaluate(ch)
