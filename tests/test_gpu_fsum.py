"""zk_mle_fraction_tree / zk_fsum_prove / zk_fsum_verify_host / zk_lookup_multiplicities / zk_bench_fsum on the device.  The reference has
no fractional-sum argument: tests/fsum_ref.py is the definition.  In child processes under ZK_FSUM_TREE_FUSE (the levels of the fraction
tree per launch): every proof of the shared case list -- sum, proof, point and claims -- byte for byte against the definition, on every
setting; both heaps of every tree from 2 elements to two levels past the LDS stage on the three fields against Python integers; on BN254
the tree over 2^20 elements, and with one level per launch over the smallest table at which the capped grid takes a second trip, against
the C oracle's arithmetic.  In the parent: the prover's shape [3, 3] at degree 3 through the public sumcheck call, one proof on the
workload's own scale (2^20), the multiplicities against the definition, repeated calls over stale pool blocks, the error table, the
measurement hook, the C++ mirror and a lookup made of public calls only."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from oracle import gkr_ref
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import gkr
from zk_amd._lib import c, lib, u8p, u64p

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsum_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from fsum_check import BIG_SEED, BIG_VARS, FIELD_IDS, SETTINGS, SWITCH, TREE_KINDS, big_vars, case_key, digest, oracle_heaps, tree_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "fsum_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BAD, MISMATCH = -20, -26


@pytest.fixture(scope="module")
def children():
    """{setting: {(kind, field id, key): digest}}: one child process per switch setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"fsum {setting} ok" in r.stdout
        lines = [ln.split() for ln in r.stdout.splitlines()]
        out[setting] = {(ln[0], ln[1], ln[2]): ln[3] for ln in lines if ln and ln[0] in ("TREE", "BIGTREE", "PROOF")}
    return out


@pytest.fixture(scope="module")
def expected():
    """the definition's digests, computed once: {("PROOF", field id, key): ..} and {("TREE", field id, key): ..}"""
    out = {}
    for case in ref.GPU_CASES:
        fi, q, p_tab, shift, seed = ref.case_inputs(case, worst_case_values)
        total, proof, point, claims = ref.prove(fi, q, seed, p_tab, shift)
        got = ref.verify(fi, case[0], p_tab is not None, seed, total, proof, shift)
        assert (got is None and total[1] == 0) if case[2] == "cancel" else got == (point, claims), case
        out[("PROOF", FIELD_IDS[fi], case_key(case))] = digest(orc.from_ints(fi, list(total)).tobytes() + proof + orc.from_ints(fi, point).tobytes()
                                                               + orc.from_ints(fi, list(claims)).tobytes())
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for n in ref.TREE_VARS:
            q, p_tab = tree_case(fi, n, p)
            for sname, pname in TREE_KINDS:
                hp, hq = ref.fraction_tree(q, p_tab if pname == "given" else None, None if sname == "null" else p - 1, p)
                out[("TREE", FIELD_IDS[fi], "n%d_%s_%s" % (n, sname, pname))] = digest(orc.from_ints(field, hp).tobytes() + orc.from_ints(field, hq).tobytes())
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_proof_on_every_setting(children, expected, setting):
    """sum, proof, point and claims of zk_fsum_prove against fsum_ref.prove, byte for byte, with 1 and 2 levels of the tree per launch and
    by default; zk_fsum_verify_host accepted each in the child (with the prover's point and claims, which are the tables' evaluations),
    fsum_ref.verify in the fixture; the case with a zero denominator is proven with D = 0 and rejected by both.  The extras take 1, 2, 3
    and 4 levels above the LDS stage: every arity of the fused kernel, then two launches"""
    want = {key: dg for key, dg in expected.items() if key[0] == "PROOF"}
    got = {key: dg for key, dg in children[setting].items() if key[0] == "PROOF"}
    assert len(want) == len(ref.GPU_CASES) and set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, (setting, wrong[:20], len(wrong))


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_trees_against_python_integers(children, expected, setting):
    """zk_mle_fraction_tree on all three fields at every size from n = 1 to two past the LDS stage, shift NULL and p - 1, p NULL and
    given; the child also compared the Q heap with zk_mle_product_tree bit for bit"""
    want = {key: dg for key, dg in expected.items() if key[0] == "TREE"}
    got = {key: dg for key, dg in children[setting].items() if key[0] == "TREE"}
    assert len(want) == 3 * 4 * len(ref.TREE_VARS) and set(got) == set(want)
    wrong = sorted(key for key in want if got[key] != want[key])
    assert not wrong, (setting, wrong)


@pytest.fixture(scope="module")
def oracle_digests():
    """{n: (digest of the C oracle's two heaps over its generator's table, N, D)}, one per size, shared by the settings"""
    out = {}
    for n in sorted({n for setting in SETTINGS for n in big_vars(setting)}):
        hp, hq = oracle_heaps(orc, FIELDS[0], orc.fill_random(FIELDS[0], BIG_SEED + n, 1 << n))
        out[n] = (digest(hp.tobytes() + hq.tobytes()), hp[1].copy(), hq[1].copy())
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_trees_against_the_oracle(children, oracle_digests, setting):
    """BN254 at 2^20 elements on every setting: every level of both heaps against the C oracle's products and sums.  With one level per
    launch also the smallest table at which the grid cap makes a wave take a second run (fsum_ref.SECOND_TRIP_VARS)"""
    sizes = big_vars(setting)
    assert sizes == ((BIG_VARS, ref.SECOND_TRIP_VARS[1]) if setting == "fuse1" else (BIG_VARS,)) and ref.SECOND_TRIP_VARS[1] == 24
    got = {key: dg for key, dg in children[setting].items() if key[0] == "BIGTREE"}
    assert set(got) == {("BIGTREE", FIELD_IDS[0], "n%d" % n) for n in sizes}
    for n in sizes:
        assert got[("BIGTREE", FIELD_IDS[0], "n%d" % n)] == oracle_digests[n][0], (setting, n)


_ctx = {}


def ctx_for(field):
    if field not in _ctx:
        _ctx[field] = zk_amd.Context(field, 0)
    return _ctx[field]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 5, 10, 12])
def test_shape_3_3_at_degree_3_through_the_public_prover(field, n):
    """the layer sumcheck's shape -- two terms of three tables, degree 3 -- through zk_sumcheck_prove_terms against the big-int model,
    before the chained use relies on it (tests/test_gpu_gkr.py's list does not hold it)"""
    ctx = ctx_for(field)
    p = zk_amd.modulus(field)
    rng = random.Random(n * 1000 + 63)
    tabs = [[[rng.randrange(p) for _ in range(1 << n)] for _ in range(3)] for _ in range(2)]
    s = sum(t[0][j] * t[1][j] % p * t[2][j] for t in tabs for j in range(1 << n)) % p
    want_rp, want_ch, want_fin = gkr_ref.prove_partial_terms(field, tabs, 3, s)
    poly = gkr.SumOfProductsPoly([[MLE.new(ctx, n, zk_amd.fe_from_ints(field, t)) for t in term] for term in tabs])
    rp, ch, fin = gkr.prove_partial_terms(poly, 3, zk_amd.fe_from_int(field, s))
    ints = lambda a: zk_amd.fe_to_ints(field, np.asarray(a).reshape(-1, 4))
    assert [ints(r) for r in rp] == want_rp and ints(ch) == want_ch and ints(fin) == want_fin
    assert ints(poly.terms[1][2].evaluation_slice()) == tabs[1][2]   # not consumed


def test_one_proof_on_the_workloads_scale(oracle_digests):
    """BN254, n = 20, on orc.fill_random's tables: the chained big rounds exist only above the finisher sizes.  zk_fsum_verify_host and
    the definition's verifier accept with the same point and claims; (N, D) are the oracle's tree's for p = ones, and the proof with a
    given p leaves the oracle's evaluations of p and q; both tables are bit-identical afterwards"""
    field, n = FIELDS[0], BIG_VARS
    ctx = ctx_for(field)
    q, pt = MLE.random(ctx, n, BIG_SEED + n), MLE.random(ctx, n, BIG_SEED + n + 100)
    q_tab, p_tab = orc.fill_random(field, BIG_SEED + n, 1 << n), orc.fill_random(field, BIG_SEED + n + 100, 1 << n)
    seed = bytes(range(32))
    for p_arg, p_src in ((None, None), (pt, p_tab)):
        total, proof, point, claims = zk_amd.fractional_sum_prove(q, seed, p_arg)
        got = zk_amd.fractional_sum_verify(field, n, p_arg is not None, seed, total, proof)
        assert got is not None and np.array_equal(got[0], point) and np.array_equal(got[1], claims)
        want = ref.verify(field, n, p_arg is not None, seed, tuple(orc.to_ints(field, total)), proof)
        assert want is not None and want[0] == orc.to_ints(field, point) and list(want[1]) == orc.to_ints(field, claims)
        assert np.array_equal(orc.mle_evaluate(field, n, q_tab, point), claims[1])
        if p_src is None:
            assert np.array_equal(total[0], oracle_digests[n][1]) and np.array_equal(total[1], oracle_digests[n][2])
            assert np.array_equal(claims[0], orc.from_int(field, 1))
        else:
            assert np.array_equal(orc.mle_evaluate(field, n, p_src, point), claims[0])
    assert np.array_equal(q.evaluation_slice(), q_tab) and np.array_equal(pt.evaluation_slice(), p_tab)
    q.free()
    pt.free()


# ---- multiplicities ----------------------------------------------------------------------------------------------------------------------
def _keys(arr):
    """the 256-bit keys of an (n, 4) limb array as Python integers: what the device compares"""
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(arr, dtype="<u8")]


def _check_mult(ctx, field, table, witness):
    """zk_lookup_multiplicities on two limb arrays against the definition; returns the definition's result"""
    m_vars, n_vars = table.shape[0].bit_length() - 1, witness.shape[0].bit_length() - 1
    t, w = MLE.new(ctx, m_vars, table), MLE.new(ctx, n_vars, witness)
    want = ref.multiplicities(_keys(table), _keys(witness))
    m, missing, first_missing, duplicates = zk_amd.lookup_multiplicities(t, w)
    assert (missing, first_missing, duplicates) == want[1:], (m_vars, n_vars, (missing, first_missing, duplicates), want[1:])
    assert m.n_vars() == m_vars and np.array_equal(m.evaluation_slice(), orc.from_ints(field, want[0]))
    assert np.array_equal(t.evaluation_slice(), table) and np.array_equal(w.evaluation_slice(), witness)
    for x in (t, w, m):
        x.free()
    return want


def _mult_tables(field, m_vars, n_vars, kind, rng):
    p = orc.modulus(field)
    rows, entries = 1 << m_vars, 1 << n_vars
    vals = list(dict.fromkeys(rng.randrange(3, 1 << 200) for _ in range(rows + 4)))   # distinct
    assert len(vals) == rows + 4
    table_vals, absent = vals[:rows], vals[rows:]
    if kind == "permutation":   # every row the same number of times (or at most one more), in a shuffled order
        witness_vals = [table_vals[i % rows] for i in range(entries)]
        rng.shuffle(witness_vals)
    elif kind == "all_equal":   # the contention case: one counter takes every add
        witness_vals = [table_vals[rng.randrange(rows)]] * entries
    elif kind == "missing":
        witness_vals = [rng.choice(table_vals) for _ in range(entries)]
        for i in rng.sample(range(entries), min(entries, 3)):
            witness_vals[i] = rng.choice(absent)
    elif kind == "duplicates":   # equal table values: the lowest index gets the count
        table_vals = [table_vals[rng.randrange(max(1, rows // 3))] for _ in range(rows)]
        witness_vals = [rng.choice(table_vals + absent[:1]) for _ in range(entries)]
    elif kind == "edges":        # worst-case limbs, 0 and p - 1
        pool = list(dict.fromkeys([0, p - 1, 1] + [x % p for x in worst_case_values(p, FIELDS.index(field), 256)]))
        table_vals = [pool[i % len(pool)] for i in range(rows)]
        witness_vals = [rng.choice(pool) for _ in range(entries)]
    else:
        raise AssertionError(kind)
    return orc.from_ints(field, table_vals), orc.from_ints(field, witness_vals)


@pytest.mark.parametrize("n_vars", [0, 3, 10, 14])
@pytest.mark.parametrize("m_vars", [0, 1, 5, 10, 12])
def test_multiplicities_against_the_definition(m_vars, n_vars):
    field = FIELDS[(m_vars + n_vars) % 3]
    ctx = ctx_for(field)
    rng = random.Random(0x10C + 100 * m_vars + n_vars)
    seen = set()
    for kind in ("permutation", "all_equal", "missing", "duplicates", "edges"):
        want = _check_mult(ctx, field, *_mult_tables(field, m_vars, n_vars, kind, rng))
        seen.add((want[1] > 0, want[3] > 0))
        if kind == "permutation":
            assert want[1] == 0 and want[3] == 0 and set(want[0]) <= {(1 << n_vars) >> m_vars, ((1 << n_vars) >> m_vars) + 1}
        if kind == "all_equal":
            assert sorted(want[0])[-1] == 1 << n_vars and sum(want[0]) == 1 << n_vars
        if kind == "missing":
            assert want[1] == min(1 << n_vars, 3) and want[2] < 1 << n_vars
    assert (True, False) in seen and (False, False) in seen and (m_vars < 2 or any(d for _, d in seen))


@pytest.mark.parametrize("word", [0, 7])
def test_multiplicities_of_keys_that_differ_in_one_word(word):
    """keys that agree in seven of their eight 32-bit words: only the lowest, or only the highest, tells them apart (the compare is on all
    eight, and the hash mixes all eight).  The limbs are given raw: every one is below p"""
    field = FIELDS[0]
    ctx = ctx_for(field)
    rng = random.Random(77 + word)
    base = np.frombuffer(rng.randrange(1 << 250).to_bytes(32, "little"), dtype="<u4").copy()
    base[7] &= 0x0FFFFFF   # far below every modulus, whatever word 7 becomes below
    rows = 1 << 10
    table = np.tile(base, (rows, 1))
    table[:, word] = (np.arange(rows, dtype=np.uint32) * (0x9E3779B1 if word == 0 else 1)) + (0 if word == 0 else 5)
    table = np.ascontiguousarray(table).view("<u8").reshape(rows, 4)
    assert all(k < orc.modulus(field) for k in _keys(table[[0, rows - 1]])) and len(set(_keys(table))) == rows
    idx = np.array([rng.randrange(rows) for _ in range(1 << 12)])
    witness = table[idx].copy()
    absent = np.ascontiguousarray(table[3]).view("<u4").copy()
    absent[word] ^= 0x00800000   # differs from row 3 in that word only, and from every row
    witness[17] = absent.view("<u8")
    want = _check_mult(ctx, field, table, witness)
    assert want[1:] == (1, 17, 0)


def test_multiplicities_large_and_second_grid_trip():
    """BN254, a table of 2^16 rows and a witness of 2^20 entries -- the smallest witness at which a thread of the count kernel takes a
    second entry (fsum_ref.MULT_SECOND_TRIP_VARS): witness[i] = table[i mod 2^16], so every count is 2^4; then entries drawn at random
    with some absent ones, counted with numpy"""
    field, m_vars, n_vars = FIELDS[0], 16, ref.MULT_SECOND_TRIP_VARS
    assert n_vars == 20 and (1 << n_vars) == 2 * ref.MAX_BLOCKS * ref.THREADS
    ctx = ctx_for(field)
    rows, entries = 1 << m_vars, 1 << n_vars
    table = orc.fill_random(field, 0x7AB1E, rows)
    assert len(set(_keys(table))) == rows
    t = MLE.new(ctx, m_vars, table)
    w = MLE.new(ctx, n_vars, np.tile(table, (entries // rows, 1)))
    m, missing, first_missing, duplicates = zk_amd.lookup_multiplicities(t, w)
    assert (missing, first_missing, duplicates) == (0, ref.NONE_MISSING, 0)
    assert np.array_equal(m.evaluation_slice(), np.tile(orc.from_int(field, entries // rows), (rows, 1)))
    m.free()
    w.free()
    rng = np.random.default_rng(9)
    idx = rng.integers(0, rows, entries)
    witness = table[idx].copy()
    gone = np.sort(rng.choice(entries, 5, replace=False))
    witness[gone, 0] ^= np.uint64(1)   # the lowest word flipped: with overwhelming probability in no row
    assert not set(_keys(witness[gone])) & set(_keys(table))
    counts = np.bincount(np.delete(idx, gone), minlength=rows)
    w = MLE.new(ctx, n_vars, witness)
    first = zk_amd.lookup_multiplicities(t, w)
    assert first[1:] == (5, int(gone[0]), 0)
    got = first[0].evaluation_slice().copy()
    small = {int(v): orc.from_int(field, int(v)) for v in np.unique(counts)}
    assert np.array_equal(got, np.stack([small[int(v)] for v in counts]))
    # after pool churn the same bytes
    first[0].free()
    for k in list(range(0, 18)) * 2:
        MLE.random(ctx, k, 5 + k).free()
    again = zk_amd.lookup_multiplicities(t, w)
    assert again[1:] == first[1:] and np.array_equal(again[0].evaluation_slice(), got)
    assert np.array_equal(t.evaluation_slice(), table) and np.array_equal(w.evaluation_slice(), witness)
    for x in (again[0], t, w):
        x.free()


@pytest.fixture(params=range(3), ids=FIELD_IDS)
def fctx(request):
    return request.param, FIELDS[request.param], ctx_for(FIELDS[request.param])


def test_repeated_calls_over_stale_pool_blocks(fctx):
    """two calls give identical bytes after random tables of the scratch's size classes have been allocated and freed, and p and q are
    bit-identical after tree and proof"""
    fi, field, ctx = fctx
    p = orc.modulus(field)
    n = 12
    q_int, p_int = tree_case(fi, n, p)
    src_q, src_p = orc.from_ints(field, q_int), orc.from_ints(field, p_int)
    shift = orc.from_int(field, 3)
    q, pt = MLE.new(ctx, n, src_q), MLE.new(ctx, n, src_p)
    first = zk_amd.fractional_sum_prove(q, bytes(32), pt, shift)
    first_ones = zk_amd.fractional_sum_prove(q, bytes(32), None, shift)
    heaps = zk_amd.fraction_tree(q, pt, shift)
    first_heaps = [h.evaluation_slice().copy() for h in heaps]
    for h in heaps:
        h.free()
    for n_vars in list(range(0, 14)) * 2:
        MLE.random(ctx, n_vars, 31 + n_vars).free()
    for before, p_arg in ((first, pt), (first_ones, None)):
        again = zk_amd.fractional_sum_prove(q, bytes(32), p_arg, shift)
        assert before[1] == again[1] and all(np.array_equal(a, b) for a, b in zip(before[::2], again[::2])) and np.array_equal(before[3], again[3])
    heaps = zk_amd.fraction_tree(q, pt, shift)
    assert all(np.array_equal(h.evaluation_slice(), f) for h, f in zip(heaps, first_heaps))
    assert np.array_equal(first_heaps[0][1], first[0][0]) and np.array_equal(first_heaps[1][1], first[0][1])
    for h in heaps:
        h.free()
    assert np.array_equal(q.evaluation_slice(), src_q) and np.array_equal(pt.evaluation_slice(), src_p)
    want = ref.prove(field, q_int, bytes(32), p_int, 3)
    assert (tuple(orc.to_ints(field, first[0])), first[1]) == want[:2]
    q.free()
    pt.free()


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    n = 6
    q, pt, q_other, q0, q5 = MLE.random(ctx, n, 1), MLE.random(ctx, n, 2), MLE.random(other, n, 1), MLE.random(ctx, 0, 2), MLE.random(ctx, n - 1, 3)
    before_q, before_p = q.evaluation_slice().copy(), pt.evaluation_slice().copy()
    raw_p = np.frombuffer(p.to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    pp = raw_p.ctypes.data_as(u64p)
    hp, hq = c.c_void_p(), c.c_void_p()
    tr = lib.zk_mle_fraction_tree
    # NULL (p and the shift may be), another context, n, p's n, the shift -- in this order
    assert tr(None, None, q._h, None, c.byref(hp), c.byref(hq)) == BAD and tr(ctx._h, pt._h, None, None, c.byref(hp), c.byref(hq)) == BAD
    assert tr(ctx._h, None, q._h, None, None, c.byref(hq)) == BAD and tr(ctx._h, None, q._h, None, c.byref(hp), None) == BAD
    assert tr(ctx._h, None, q_other._h, pp, c.byref(hp), c.byref(hq)) == MISMATCH and tr(other._h, None, q._h, None, c.byref(hp), c.byref(hq)) == MISMATCH
    assert tr(ctx._h, q_other._h, q._h, pp, c.byref(hp), c.byref(hq)) == MISMATCH
    assert tr(ctx._h, None, q0._h, pp, c.byref(hp), c.byref(hq)) == BAD and tr(ctx._h, q5._h, q._h, None, c.byref(hp), c.byref(hq)) == BAD
    assert tr(ctx._h, pt._h, q._h, pp, c.byref(hp), c.byref(hq)) == BAD
    assert not hp.value and not hq.value
    seed = np.arange(32, dtype=np.uint8)
    sp = seed.ctypes.data_as(u8p)
    buf = np.full(ref.proof_bytes(n), 7, dtype=np.uint8)
    total, point, claims = (np.full(s, 9, dtype=np.uint64) for s in (8, 4 * n, 8))
    bp, tp, zp, cp = buf.ctypes.data_as(u8p), total.ctypes.data_as(u64p), point.ctypes.data_as(u64p), claims.ctypes.data_as(u64p)
    pv = lib.zk_fsum_prove
    good = [ctx._h, pt._h, q._h, None, sp, tp, bp, zp, cp]
    for i in (0, 2, 4, 5, 6, 7, 8):   # every pointer but p and the shift
        bad = list(good)
        bad[i] = None
        assert pv(*bad) == BAD, i
    assert pv(other._h, pt._h, q._h, pp, sp, tp, bp, zp, cp) == MISMATCH and pv(ctx._h, None, q_other._h, None, sp, tp, bp, zp, cp) == MISMATCH
    assert pv(ctx._h, None, q0._h, pp, sp, tp, bp, zp, cp) == BAD                     # n = 0 before the shift
    assert pv(ctx._h, q5._h, q._h, None, sp, tp, bp, zp, cp) == BAD                   # p and q of different sizes
    assert pv(ctx._h, pt._h, q._h, pp, sp, tp, bp, zp, cp) == BAD                     # a shift that is not reduced
    assert (buf == 7).all() and (total == 9).all() and (point == 9).all() and (claims == 9).all()   # nothing was written by any of them
    assert pv(*good) == 0
    want = ref.prove(field, orc.to_ints(field, before_q), seed.tobytes(), orc.to_ints(field, before_p))
    assert (tuple(orc.to_ints(field, total.reshape(2, 4))), buf.tobytes(), orc.to_ints(field, point.reshape(n, 4)),
            tuple(orc.to_ints(field, claims.reshape(2, 4)))) == want
    # multiplicities: NULLs, another context; nothing written
    lm = lib.zk_lookup_multiplicities
    h = c.c_void_p()
    cnt = [c.c_uint64(77) for _ in range(3)]
    refs = [c.byref(x) for x in cnt]
    good = [ctx._h, q._h, q5._h, c.byref(h)] + refs
    for i in range(7):
        bad = list(good)
        bad[i] = None
        assert lm(*bad) == BAD, i
    assert lm(ctx._h, q_other._h, q5._h, c.byref(h), *refs) == MISMATCH and lm(ctx._h, q._h, q_other._h, c.byref(h), *refs) == MISMATCH
    assert not h.value and all(x.value == 77 for x in cnt)
    # the measurement hook gives a time on its four paths and leaves the table alone
    ms = c.c_double(-1.0)
    for path in (0, 1, 2, 3):
        ms.value = -1.0
        assert lib.zk_bench_fsum(ctx._h, q._h, path, 2, c.byref(ms)) == 0 and ms.value > 0, path
    assert zk_amd.bench_fsum(q, path=2, reps=1) > 0
    ms.value = -1.0
    assert lib.zk_bench_fsum(ctx._h, q._h, 4, 1, c.byref(ms)) == BAD and lib.zk_bench_fsum(ctx._h, q._h, 0, 0, c.byref(ms)) == BAD
    assert lib.zk_bench_fsum(ctx._h, q._h, 0, 1, None) == BAD and lib.zk_bench_fsum(ctx._h, None, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_fsum(other._h, q._h, 0, 1, c.byref(ms)) == MISMATCH and lib.zk_bench_fsum(ctx._h, q0._h, 0, 1, c.byref(ms)) == BAD
    assert ms.value == -1.0 and np.array_equal(q.evaluation_slice(), before_q) and np.array_equal(pt.evaluation_slice(), before_p)
    ctx.close()
    other.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_fsum.cpp over zk.hpp: trees, proofs, the verifier's verdicts, the multiplicities, the errors"""
    exe = str(tmp_path / "test_fsum")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fsum.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: fsum host tests passed" in r.stdout


def test_lookup_from_public_calls():
    """every entry of f occurs in t: f, t and the multiplicities m are committed, alpha is drawn from a transcript over the three roots,
    lookup_prove / lookup_verify run on a seed that binds them, and the three claims the proofs leave are opened from the commitments at
    the returned points.  With one witness entry outside the table lookup_prove raises, and a forged m is rejected"""
    field, n_f, n_t, blowup, log_final, queries = zk_amd.BN254_FR, 7, 5, 1, 0, 8
    p = orc.modulus(field)
    ctx = zk_amd.Context(field, 0)
    rng = np.random.default_rng(11)
    t_vals = [int(x) for x in rng.choice(1 << 20, 1 << n_t, replace=False)]
    f_vals = [t_vals[i] for i in rng.integers(0, 1 << n_t, 1 << n_f)]
    one = orc.from_int(field, 1)
    f, t = (MLE.new(ctx, n, orc.from_ints(field, v)) for n, v in ((n_f, f_vals), (n_t, t_vals)))
    m, missing, _, duplicates = zk_amd.lookup_multiplicities(t, f)
    assert missing == 0 and duplicates == 0
    assert orc.to_ints(field, m.evaluation_slice()) == ref.multiplicities(t_vals, f_vals)[0]
    coms = [zk_amd.MultilinearCommitment.commit(x, blowup, one) for x in (f, t, m)]
    roots = [com.root() for com in coms]
    tr = zk_amd.Transcript()
    tr.append(b"".join(roots))
    alpha = tr.sample_field_element(field)        # after the three commitments
    seed = zk_amd.keccak256(b"".join(roots))      # binds witness, table and multiplicities
    m2, proof = zk_amd.lookup_prove(f, t, alpha, seed)
    assert np.array_equal(m2.evaluation_slice(), m.evaluation_slice())
    got = zk_amd.lookup_verify(field, n_f, n_t, alpha, seed, proof)
    assert got is not None
    (r_f, f_claim), (r_t, t_claim, m_claim) = got
    a = orc.to_int(field, alpha)
    want = ref.lookup_prove(field, f_vals, t_vals, a, seed)
    assert (tuple(orc.to_ints(field, proof[0])), proof[1], tuple(orc.to_ints(field, proof[2])), proof[3]) == want[1]
    want_out = ref.lookup_verify(field, n_f, n_t, a, seed, want[1])
    assert want_out == ((orc.to_ints(field, r_f), orc.to_int(field, f_claim)),
                        (orc.to_ints(field, r_t), orc.to_int(field, t_claim), orc.to_int(field, m_claim)))
    for com, root, point, claim in ((coms[0], roots[0], r_f, f_claim), (coms[1], roots[1], r_t, t_claim), (coms[2], roots[2], r_t, m_claim)):
        value, opening = com.open(point, log_final, queries, seed)
        assert np.array_equal(value, claim)
        assert zk_amd.mlpcs_verify(field, root, point, claim, opening, blowup, log_final, queries, one, seed)
    # a forged m: one count moved from one row to another (the sum of m is unchanged, the fractional sums differ)
    m_vals = orc.to_ints(field, m.evaluation_slice())
    hit = next(j for j, v in enumerate(m_vals) if v)
    m_vals[hit], m_vals[(hit + 1) % len(m_vals)] = m_vals[hit] - 1, m_vals[(hit + 1) % len(m_vals)] + 1
    forged = MLE.new(ctx, n_t, orc.from_ints(field, m_vals))
    sf, st = ref.lookup_seeds(seed)
    total_t, proof_t, _, _ = zk_amd.fractional_sum_prove(t, st, forged, alpha)
    assert zk_amd.fractional_sum_verify(field, n_t, True, st, total_t, proof_t, alpha) is not None   # a true statement about the forged m
    assert zk_amd.lookup_verify(field, n_f, n_t, alpha, seed, (proof[0], proof[1], total_t, proof_t)) is None
    # one witness entry outside the table
    f_vals[41] = (1 << 20) + 5
    f_bad = MLE.new(ctx, n_f, orc.from_ints(field, f_vals))
    with pytest.raises(ValueError, match=r"witness entry 41 \(first_missing\)"):
        zk_amd.lookup_prove(f_bad, t, alpha, seed)
    for x in [f, t, m, m2, forged, f_bad] + coms:
        x.free()
    ctx.close()
