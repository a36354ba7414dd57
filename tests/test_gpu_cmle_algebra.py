"""The algebra of device-resident coefficient-form multilinear polynomials (zk_cmle_partial_evaluate / _relabel / _scalar_multiply / _add /
_mul; coefficient_form.rs :72-123, :272-282, :350-415) on the GPU, bit for bit against the dict model that follows the reference loop
for loop (tests/cmle_algebra_ref.py): which keys are present, their coefficients, n_vars and to_bytes.  Larger sizes against a numpy
object-array contraction (2^16) and against the oracle-pinned evaluator (2^20, 2^22).  Mul keeps the keys the reference drops for zero
coefficients, as zeros: with zeros planted the model's missing keys are zero-filled before comparing, and only there."""
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import DeviceCoeffMultilinear as DC
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import ZkError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cmle_algebra_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
SELECTOR_LEN, SELECTOR_SINGLE, UNSUPPORTED = -13, -14, -25


@pytest.fixture(params=FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def fctx(request):
    ctx = zk_amd.Context(request.param, 0)
    yield request.param, ctx
    ctx.close()


@pytest.fixture
def bn():
    ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
    yield zk_amd.BN254_FR, ctx
    ctx.close()


def _fe(field, x):
    return orc.from_ints(field, [x])[0]


def _dense(field, ctx, n, seed):
    """a device polynomial with every key and its model (n, {key: int})"""
    co = orc.fill_random(field, seed, 1 << n)
    return DC.upload(ctx, n, co), (n, dict(enumerate(orc.to_ints(field, co))))


def _upload(field, ctx, n, ints):
    return DC.upload(ctx, n, orc.from_ints(field, ints)), (n, dict(enumerate(ints)))


def _assign(field, n, pairs):
    """[(variable, int)] -> the device's and the model's assignment lists"""
    return [(ref.selector(n, v), _fe(field, r)) for v, r in pairs], [(ref.selector(n, v), r) for v, r in pairs]


def _same(field, d, model):
    """the device polynomial is the model: n_vars, the present keys, their coefficients, the serialisation"""
    n, co = model
    keys = sorted(co)
    assert d.n_vars() == n
    assert len(d) == len(keys) and [int(k) for k in d.keys()] == keys
    assert orc.to_ints(field, d.coefficients()) == [co[k] for k in keys]
    assert d.to_bytes() == ref.to_bytes(model)


def _values(field, rng, count):
    p = orc.modulus(field)
    return [rng.choice([0, 1, p - 1]) if rng.random() < 0.4 else rng.randrange(p) for _ in range(count)]


def test_partial_evaluate_every_subset_of_four(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(4)
    d, model = _dense(field, ctx, 4, 0xA4)
    for size in range(5):
        for subset in itertools.combinations(range(4), size):
            pairs = list(zip(subset, _values(field, rng, size)))
            rng.shuffle(pairs)
            dev, mod = _assign(field, 4, pairs)
            got = d.partial_evaluate(dev)
            assert got.fixed_mask() == sum(1 << v for v in subset)
            _same(field, got, ref.partial_evaluate(model, mod, p))
    _same(field, d, model)   # out of place


def _variable_sets(n, s, rng):
    sets = [list(range(s)), list(range(n - s, n)), sorted(rng.sample(range(n), s))]
    if s >= 2:
        sets.append([0] + sorted(rng.sample(range(3, n), s - 1)))   # one low variable among high ones
    return sets


@pytest.mark.parametrize("n", [11, 12, 14])
def test_partial_evaluate_groups_and_positions(fctx, n):
    """s = 1, 2, 3, 4, 7 newly fixed variables: passes of three with a remainder of 1, 2 and 0; lowest, highest and mixed
    positions"""
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(n)
    d, model = _dense(field, ctx, n, 0xB00 + n)
    for s in [1, 2, 3, 4, 7]:
        for subset in _variable_sets(n, s, rng):
            pairs = list(zip(subset, _values(field, rng, s)))
            rng.shuffle(pairs)
            dev, mod = _assign(field, n, pairs)
            _same(field, d.partial_evaluate(dev), ref.partial_evaluate(model, mod, p))


def _contract(ints, n, pairs, p):
    """numpy object arrays: axis n-1-v of the reshaped vector is key bit v; the highest variable first, so the others keep their axes"""
    a = np.array(ints, dtype=object).reshape([2] * n)
    for v, r in sorted(pairs, reverse=True):
        ax = a.ndim - 1 - v
        a = (a.take(0, axis=ax) + a.take(1, axis=ax) * r) % p
    return [int(x) for x in a.reshape(-1)]


def test_partial_evaluate_2p16_against_numpy(bn):
    field, ctx = bn
    p = orc.modulus(field)
    rng = random.Random(16)
    n = 16
    co = orc.fill_random(field, 0x1616, 1 << n)
    d, ints = DC.upload(ctx, n, co), orc.to_ints(field, co)
    assert _contract(orc.to_ints(field, orc.fill_random(field, 1, 16)), 4, [], p) == orc.to_ints(field, orc.fill_random(field, 1, 16))
    for subset in [[0, 1, 2], [13, 14, 15], [0, 1, 2, 3, 4, 5, 6, 7], sorted(rng.sample(range(n), 5)), sorted(rng.sample(range(n), 10))]:
        pairs = list(zip(subset, _values(field, rng, len(subset))))
        got = d.partial_evaluate(_assign(field, n, pairs)[0])
        assert got.fixed_mask() == sum(1 << v for v in subset)
        assert orc.to_ints(field, got.coefficients()) == _contract(ints, n, pairs, p), subset


def _by_evaluation(field, ctx, n, seed, subsets):
    """partial_evaluate(S).evaluate_slice(point) == evaluate_slice(point with the assigned values at S): the evaluator is oracle-pinned"""
    rng = random.Random(seed)
    p = orc.modulus(field)
    d = DC.interpolate(ctx, MLE.random(ctx, n, seed))
    for subset in subsets:
        pairs = list(zip(subset, _values(field, rng, len(subset))))
        rng.shuffle(pairs)
        got = d.partial_evaluate(_assign(field, n, pairs)[0])
        assert len(got) == 1 << (n - len(subset))
        point = [rng.randrange(p) for _ in range(n)]
        merged = list(point)
        for v, r in pairs:
            merged[v] = r
        want = d.evaluate_slice(orc.from_ints(field, merged))
        assert np.array_equal(got.evaluate_slice(orc.from_ints(field, point)), want), subset   # the fixed coordinates are ignored
        assert np.array_equal(got.relabel().evaluate_slice(orc.from_ints(field, [point[v] for v in range(n) if v not in subset])), want)
        got.free()


def test_partial_evaluate_2p20_by_evaluation(fctx):
    field, ctx = fctx
    _by_evaluation(field, ctx, 20, 0x2020, [[0, 1, 2], [17, 18, 19], [0, 3, 7, 11, 12, 16, 19]])


def test_partial_evaluate_2p22_by_evaluation_bn254(bn):
    field, ctx = bn
    _by_evaluation(field, ctx, 22, 0x2222, [[0, 1, 2], [19, 20, 21], [1, 2, 5, 9, 13, 17, 21], list(range(22))])


def test_chaining_and_assignment_rules(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    n = 12
    d, model = _dense(field, ctx, n, 0xC4)
    dev1, mod1 = _assign(field, n, [(3, 5), (0, p - 1), (11, 77)])
    first, m1 = d.partial_evaluate(dev1), ref.partial_evaluate(model, mod1, p)
    dev2, mod2 = _assign(field, n, [(1, 9), (3, 1234), (10, 0), (2, 3)])   # variable 3 is fixed already: nothing happens
    second, m2 = first.partial_evaluate(dev2), ref.partial_evaluate(m1, mod2, p)
    assert second.fixed_mask() == 0b110000001111
    _same(field, second, m2)
    _same(field, first, m1)   # the masked input is left as it was
    dev3, mod3 = _assign(field, n, [(4, 2), (4, 3), (5, 4), (4, 5)])   # repeated: the first value of a variable wins
    _same(field, d.partial_evaluate(dev3), ref.partial_evaluate(model, mod3, p))
    _same(field, d.partial_evaluate(dev3), ref.partial_evaluate(model, _assign(field, n, [(4, 2), (5, 4)])[1], p))
    longer = ([False] * n + [True], _fe(field, 3))   # a selector longer than n_vars is ignored
    _same(field, d.partial_evaluate([longer]), model)
    _same(field, d.partial_evaluate([longer] + dev1), m1)
    copy = d.partial_evaluate([])
    _same(field, copy, model)
    _same(field, first.partial_evaluate([]), m1)
    for bad, code, text in [([True] + [False] * (n - 2), SELECTOR_LEN, ref.SELECTOR_LEN_TEXT), ([], SELECTOR_LEN, ref.SELECTOR_LEN_TEXT),
                            ([False] * n, SELECTOR_SINGLE, ref.SELECTOR_SINGLE_TEXT),
                            ([True, True] + [False] * (n - 2), SELECTOR_SINGLE, ref.SELECTOR_SINGLE_TEXT)]:
        for target in (d, first):
            with pytest.raises(ZkError) as e:
                target.partial_evaluate(dev1[:1] + [(bad, _fe(field, 2))])
            assert e.value.code == code and str(e.value) == text
        with pytest.raises(ValueError, match=text[:20]):
            ref.partial_evaluate(model, [(bad, 2)], p)
    # the reference stops at the first bad assignment: a short selector before one with two bits is the length error
    with pytest.raises(ZkError) as e:
        d.partial_evaluate([([True], _fe(field, 2)), ([True, True] + [False] * (n - 2), _fe(field, 2))])
    assert e.value.code == SELECTOR_LEN
    _same(field, d, model)


def test_masked_handles_and_relabel(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(9)
    for n, subset in [(5, [1, 3]), (9, [0, 8]), (12, [0, 1, 2, 6]), (13, [12]), (6, list(range(6)))]:
        d, model = _dense(field, ctx, n, 0xD00 + n)
        pairs = list(zip(subset, _values(field, rng, len(subset))))
        dev, mod = _assign(field, n, pairs)
        got, want = d.partial_evaluate(dev), ref.partial_evaluate(model, mod, p)
        _same(field, got, want)   # coefficients, keys and to_bytes of the masked handle
        host = got.to_host()
        assert host.n_vars() == n and sorted(host.coefficients) == sorted(want[1])
        point = [rng.randrange(p) for _ in range(n + 2)]
        assert orc.to_int(field, got.evaluate_slice(orc.from_ints(field, point))) == ref.evaluate_slice(want, point, p)
        with pytest.raises(ZkError) as e:
            got.evaluate_slice(orc.from_ints(field, point[:n - 1]))   # the check is on the full n_vars
        assert e.value.code == -12
        with pytest.raises(ZkError) as e:
            got.to_evaluation_form()
        assert e.value.code == UNSUPPORTED
        relabelled = ref.relabel(want, p)
        assert relabelled[0] == n - len(subset)
        assert got.relabel() is got and got.fixed_mask() == 0
        _same(field, got, relabelled)
        if relabelled[0]:
            table = got.to_evaluation_form().evaluation_slice()   # a relabelled handle is an ordinary one again
            assert orc.to_int(field, table[0]) == relabelled[1][0]
        _same(field, d, model)
    d, model = _dense(field, ctx, 7, 0xD77)
    assert ref.relabel(model, p) == model
    _same(field, d.relabel(), model)   # every variable occurs in some key: the identity
    const, cmodel = _upload(field, ctx, 0, [41])
    _same(field, const.relabel(), ref.relabel(cmodel, p))
    assert const.n_vars() == 0 and const.fixed_mask() == 0


def test_reference_relabel_example(fctx):
    """test_poly_relabelling (:1192-1245) with every key present: 2ab + 3cd + 5acd + 6bd at b = c = 1 -> 2a + 9d + 5ad -> 2a + 9b + 5ab"""
    field, ctx = fctx
    ints = [0] * 16
    ints[3], ints[12], ints[13], ints[10] = 2, 3, 5, 6
    d, _ = _upload(field, ctx, 4, ints)
    q = d.partial_evaluate(_assign(field, 4, [(1, 1), (2, 1)])[0])
    assert q.n_vars() == 4 and [int(k) for k in q.keys()] == [0, 1, 8, 9] and orc.to_ints(field, q.coefficients()) == [0, 2, 9, 5]
    q.relabel()
    assert q.n_vars() == 2 and [int(k) for k in q.keys()] == [0, 1, 2, 3] and orc.to_ints(field, q.coefficients()) == [0, 2, 9, 5]


def test_add(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    a, ma = _dense(field, ctx, 9, 0xE1)
    b, mb = _dense(field, ctx, 9, 0xE2)
    s, ms = _dense(field, ctx, 3, 0xE3)
    _same(field, a + b, ref.add(ma, mb, p))
    _same(field, a + s, ref.add(ma, ms, p))   # n 9 + 3: the longer one's n_vars, the shorter summed into the low keys
    _same(field, s + a, ref.add(ms, ma, p))
    neg = a.scalar_multiply(_fe(field, p - 1))
    zero = a + neg
    assert len(zero) == 512 and not zero.coefficients().any()   # every key stays, with zero
    _same(field, zero, ref.add(ma, ref.scalar_multiply(ma, p - 1, p), p))
    top, mt = _upload(field, ctx, 5, [p - 1] * 32)
    _same(field, top + top, ref.add(mt, mt, p))
    for n in [0, 1, 13]:
        x, mx = _dense(field, ctx, n, 0xE40 + n)
        y, my = _dense(field, ctx, n, 0xE50 + n)
        _same(field, x + y, ref.add(mx, my, p))
    masked = a.partial_evaluate(_assign(field, 9, [(2, 7)])[0])
    for lhs, rhs in [(masked, a), (a, masked)]:
        with pytest.raises(ZkError) as e:
            lhs + rhs
        assert e.value.code == UNSUPPORTED
    _same(field, masked.relabel() + a, ref.add(ref.relabel(ref.partial_evaluate(ma, _assign(field, 9, [(2, 7)])[1], p), p), ma, p))


def test_scalar_multiply(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(5)
    for n in [0, 1, 6, 14]:
        d, model = _dense(field, ctx, n, 0xF00 + n)
        for s in [0, 1, p - 1, rng.randrange(p)]:
            _same(field, d.scalar_multiply(_fe(field, s)), ref.scalar_multiply(model, s, p))
    d, model = _dense(field, ctx, 12, 0xF12)
    dev, mod = _assign(field, 12, [(0, 3), (7, 4), (11, 5)])
    masked, mm = d.partial_evaluate(dev), ref.partial_evaluate(model, mod, p)
    for s in [0, p - 1, rng.randrange(p)]:
        got = masked.scalar_multiply(_fe(field, s))
        assert got.fixed_mask() == masked.fixed_mask()
        _same(field, got, ref.scalar_multiply(mm, s, p))
    _same(field, masked, mm)


def _nonzero(field, rng, count):
    p = orc.modulus(field)
    return [rng.randrange(1, p) for _ in range(count)]


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (5, 7), (11, 1), (1, 11), (6, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mul_matches_the_reference_key_for_key(fctx, shape):
    """no operand coefficient is zero, so the reference skips no pair: the same keys, coefficients and bytes"""
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(shape[0] * 16 + shape[1])
    a, ma = _upload(field, ctx, shape[0], _nonzero(field, rng, 1 << shape[0]))
    b, mb = _upload(field, ctx, shape[1], _nonzero(field, rng, 1 << shape[1]))
    _same(field, a * b, ref.mul(ma, mb, p))


def test_mul_with_zero_coefficients_keeps_their_keys(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(6)
    ia, ib = _nonzero(field, rng, 32), _nonzero(field, rng, 16)
    for k in (0, 5, 31):
        ia[k] = 0
    for k in (1, 15):
        ib[k] = 0
    a, ma = _upload(field, ctx, 5, ia)
    b, mb = _upload(field, ctx, 4, ib)
    n, sparse = ref.mul(ma, mb, p)
    assert n == 9 and len(sparse) == (32 - 3) * (16 - 2)   # the reference's product lacks the keys of the skipped pairs
    _same(field, a * b, (n, {k: sparse.get(k, 0) for k in range(1 << n)}))


def test_mul_scalar_paths_and_limits(fctx):
    field, ctx = fctx
    p = orc.modulus(field)
    rng = random.Random(8)
    d, model = _upload(field, ctx, 7, _nonzero(field, rng, 128))
    for s in [rng.randrange(1, p), p - 1, 0]:
        const, cm = _upload(field, ctx, 0, [s])
        _same(field, const * d, ref.mul(cm, model, p))   # n_a == 0: rhs.scalar_multiply(key 0 of lhs), :380-381
        _same(field, d * const, ref.mul(model, cm, p))   # n_b == 0, :382-384
    c1, m1 = _upload(field, ctx, 0, [6])
    c2, m2 = _upload(field, ctx, 0, [7])
    _same(field, c1 * c2, ref.mul(m1, m2, p))
    masked = d.partial_evaluate(_assign(field, 7, [(0, 2)])[0])
    for lhs, rhs in [(masked, d), (d, masked)]:
        with pytest.raises(ZkError) as e:
            lhs * rhs
        assert e.value.code == UNSUPPORTED
    # the reference's three examples (:883-999) with every key present
    ab, _ = _upload(field, ctx, 2, [0, 0, 0, 5])
    c6, _ = _upload(field, ctx, 1, [0, 6])
    assert orc.to_ints(field, (ab * c6).coefficients()) == [0] * 7 + [30]
    lhs, _ = _upload(field, ctx, 3, [0, 0, 0, 2, 0, 3, 0, 0])
    de, _ = _upload(field, ctx, 2, [0, 0, 0, 7])
    got = orc.to_ints(field, (lhs * de).coefficients())
    assert {k: v for k, v in enumerate(got) if v} == {27: 14, 29: 21}
    x, _ = _upload(field, ctx, 4, [{1: 2, 6: 3, 8: 6}.get(k, 0) for k in range(16)])
    y, _ = _upload(field, ctx, 4, [{1: 4, 6: 5, 8: 2}.get(k, 0) for k in range(16)])
    got = orc.to_ints(field, (x * y).coefficients())
    assert {k: v for k, v in enumerate(got) if v} == {17: 8, 97: 10, 129: 4, 22: 12, 102: 15, 134: 6, 24: 24, 104: 30, 136: 12}
    two, _ = _upload(field, ctx, 2, [0, 2, 3, 0])
    c4, _ = _upload(field, ctx, 1, [0, 4])
    c5, _ = _upload(field, ctx, 1, [0, 5])
    got = orc.to_ints(field, ((two * c4) * c5).coefficients())
    assert {k: v for k, v in enumerate(got) if v} == {13: 40, 14: 60}


def test_mul_10x10_by_evaluation_and_the_size_limit(bn):
    field, ctx = bn
    p = orc.modulus(field)
    rng = random.Random(10)
    a = DC.upload(ctx, 10, orc.fill_random(field, 0xAA, 1 << 10))
    b = DC.upload(ctx, 10, orc.fill_random(field, 0xBB, 1 << 10))
    ab = a * b
    assert ab.n_vars() == 20 and len(ab) == 1 << 20
    for _ in range(3):   # (a * b)(x, y) = a(x) * b(y): a's variables come first
        x, y = [rng.randrange(p) for _ in range(10)], [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(10)]
        want = orc.to_int(field, a.evaluate_slice(orc.from_ints(field, x))) * orc.to_int(field, b.evaluate_slice(orc.from_ints(field, y))) % p
        assert orc.to_int(field, ab.evaluate_slice(orc.from_ints(field, x + y))) == want
    co = ab.coefficients()
    ia, ib = orc.to_ints(field, a.coefficients()), orc.to_ints(field, b.coefficients())
    for i, j in [(0, 0), (1023, 1023), (1, 0), (0, 1), (513, 77)]:
        assert orc.to_int(field, co[i | j << 10]) == ia[i] * ib[j] % p
    big = DC.interpolate(ctx, MLE.random(ctx, 21, 3))
    with pytest.raises(ZkError) as e:   # 21 + 20 = 41 variables: refused before anything is allocated
        big * ab
    assert e.value.code == UNSUPPORTED


def test_interpolate_restated_with_device_algebra(fctx):
    """CoeffMultilinearPolynomial::interpolate as the reference writes it (:200-237): a lagrange_basis_poly per value as a product of
    check_one / check_zero, scalar_multiply by the value, summed from the additive identity -- here with device Mul / scalar_multiply /
    Add only.  (The identity is the constant 0 with its key present; the sum's keys are those of the 3-variable terms either way.)"""
    field, ctx = fctx
    p = orc.modulus(field)
    values = orc.fill_random(field, 0x1F, 8)
    check_zero, _ = _upload(field, ctx, 1, [1, p - 1])   # 1 - a (:256-263)
    check_one, _ = _upload(field, ctx, 1, [0, 1])        # a (:266-269)
    result, _ = _upload(field, ctx, 0, [0])
    for i in range(8):
        acc, _ = _upload(field, ctx, 0, [1])             # multiplicative_identity
        for ch in format(i, "03b"):                      # binary_string(i, 3) :461-464
            acc = acc * (check_one if ch == "1" else check_zero)
        result = result + acc.scalar_multiply(values[i])
    want = DC.interpolate(ctx, values)
    assert result.n_vars() == want.n_vars() == 3 and result.fixed_mask() == 0
    assert np.array_equal(result.coefficients(), want.coefficients())
    assert result.to_bytes() == want.to_bytes()


def test_bench_hook_runs(bn):
    field, ctx = bn
    a = DC.upload(ctx, 12, orc.fill_random(field, 1, 1 << 12))
    b = DC.upload(ctx, 12, orc.fill_random(field, 2, 1 << 12))
    dev, _ = _assign(field, 12, [(0, 3), (1, 4), (2, 5), (11, 6)])
    assert a.bench_algebra(0, assignments=dev, reps=2) > 0
    assert a.bench_algebra(1, other=b, reps=2) > 0
    assert a.bench_algebra(2, scalar=_fe(field, 9), reps=2) > 0
    assert a.bench_algebra(3, other=b, reps=2) > 0
    with pytest.raises(ZkError):
        a.bench_algebra(4, reps=2)


def test_bench_cmle_wants_every_key(bn):
    """zk_bench_cmle sizes its work by n_vars, so it refuses a handle that holds fewer than 2^n_vars coefficients, and takes it again
    once it is relabelled"""
    field, ctx = bn
    d, _ = _dense(field, ctx, 6, 0xBE)
    masked = d.partial_evaluate(_assign(field, 6, [(1, 5), (4, 6)])[0])
    point = orc.fill_random(field, 3, 6)
    for op in (1, 2):
        with pytest.raises(ZkError) as e:
            masked.bench(op, point=point, reps=1)
        assert e.value.code == UNSUPPORTED
        assert d.bench(op, point=point, reps=1) > 0
    assert masked.relabel().bench(1, reps=1) > 0


def test_cpp_mirror(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_cmle_algebra")
    lib_dir = os.path.join(root, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "test_cmle_algebra.cpp"), "-L" + lib_dir,
                    "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_cmle_algebra: ok" in r.stdout, r.stdout + r.stderr
