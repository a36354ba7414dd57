"""Run by tests/test_gpu_extreme_tables.py in one child process per kernel-selecting switch set (the library reads its ZK_* switches
once per process): the raw-limb families of tests/extreme_tables.py through round_sums, prove_partial (right and wrong claim, then
consuming), prove_partial_batch, the two-term shape A.B + C, prod_reduce and partial_evaluate, every result compared bit for bit with
the CPU oracle (tests/oracle_cache.py: extreme_case, and extreme_terms_case over oracle/gkr_ref.py for the two-term shape) and, where the family has one, with its
closed form in Python integers.  Sizes come from ZK_CHECK_SIZES, fields from ZK_CHECK_FIELDS.

Cut for time: the (3, 3) shape at n >= 16 runs on BN254 only (spec() says so to the parent's prefill as well).  The two-term shape runs
at every size."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = tuple(int(x) for x in os.environ.get("ZK_CHECK_SIZES", "3,7,11").split(","))
N_FIELDS = int(os.environ.get("ZK_CHECK_FIELDS", "3"))

import numpy as np  # noqa: E402

import extreme_tables as et  # noqa: E402
import oracle_cache  # noqa: E402  (oracle answers: read from $ZK_ORACLE_CACHE when the parent test prefilled it, else computed here)
from oracle import binding as orc  # noqa: E402

KD = ((2, 2), (3, 3), (1, 1), (2, 3))
TERMS = oracle_cache.EXTREME_TERMS   # A, B, C of the two-term shape A.B + C
CHALLENGES = ("M", "O", "ONE", "Z")


def shapes(field, n):
    return tuple(kd for kd in KD if not (kd == (3, 3) and n >= 16 and field != 0))


def spec(sizes, n_fields):
    """every cached oracle answer this script needs for (sizes, n_fields): the parent prefills the cache with it"""
    return ([["ext", field, name, k, D, n] for field in range(n_fields) for n in sizes for k, D in shapes(field, n) for name in et.FAMILIES]
            + [["extterms", field, i, n] for field in range(n_fields) for n in sizes for i in range(len(TERMS))])


def expected_checks(sizes, n_fields):
    """what main() counts: per spec entry the round sums, four proofs and a batch; per (field, n) the two-term cases and, per family,
    prod_reduce and partial_evaluate"""
    n_ext = sum(1 for item in spec(sizes, n_fields) if item[0] == "ext")
    return 6 * n_ext + n_fields * len(sizes) * (len(TERMS) + 2 * len(et.FAMILIES))


EVAL_TABLES = ("const(M)", "const(O)", "step(Z,O)", "stripe(O,Z)")


def check_evaluate(ctx, field, n, oracle_points=4):
    """MLE.evaluate and ProductPoly.evaluate (the table twice) of the EVAL_TABLES at a random point, the all-zero and all-one points
    and a point whose coordinates have the representations M and O, against the closed form; the first `oracle_points` of them (counted
    from the M / O point) against the oracle's n folds as well.  -> number of evaluations compared"""
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd import ProductPoly

    raw = et.raws(field)
    points = [np.stack([et.limbs(raw["M" if i % 2 else "O"]) for i in range(n)]), orc.fill_random(field, 4900 + n, n),
              np.tile(et.limbs(raw["Z"]), (n, 1)), np.tile(et.limbs(raw["ONE"]), (n, 1))]
    done = 0
    for name in EVAL_TABLES:
        kind, a, b = et._TWO_RAW[name]
        tab = et.table(field, name, n)
        closed = et.Closed(field, n, kind, [(et.value(field, raw[a]), et.value(field, raw[b]))] * 2)
        t, u = MLE.new(ctx, n, tab), MLE.new(ctx, n, tab)
        pp = ProductPoly.new([t, u])
        for i, pt in enumerate(points):
            vals = orc.to_ints(field, pt)
            got1, got2 = t.evaluate(pt), pp.evaluate(pt)
            assert np.array_equal(got1, et.elems(field, [closed.factor(0).evaluate(vals)])[0]), ("evaluate vs closed form", field, name, n, i)
            assert np.array_equal(got2, et.elems(field, [closed.evaluate(vals)])[0]), ("product evaluate vs closed form", field, name, n, i)
            if i < oracle_points:
                assert np.array_equal(got1, orc.mle_evaluate(field, n, tab, pt)), ("evaluate vs oracle", field, name, n, i)
                assert np.array_equal(got2, orc.product_evaluate(field, n, [tab, tab], pt)), ("product evaluate vs oracle", field, name, n, i)
            done += 2
        t.free()
        u.free()
    return done


def main_eval():
    """k_eval_stream on table halves that are all ones: the parent sets ZK_EVAL_STREAM_MIN (and ZK_EVAL_WEIGHT)"""
    import zk_amd

    done = 0
    for field in (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)[:N_FIELDS]:
        ctx = zk_amd.Context(field, 0)
        for n in SIZES:
            done += check_evaluate(ctx, field, n, oracle_points=1)
    print(f"extreme evaluate ok: {done} evaluations (ZK_EVAL_STREAM_MIN={os.environ.get('ZK_EVAL_STREAM_MIN')} "
          f"ZK_EVAL_WEIGHT={os.environ.get('ZK_EVAL_WEIGHT')})")


def main_quad24():
    """k_round_quad<2,2,0> at its limit on BN254: prove_partial of T x T (one handle, listed twice) at n = 24 for T = const(O) and
    const(M).  A fused round folds first, so round 1 has 2^22 pairs; the parent's ZK_QUAD_MAX_PAIRS=2^22 gives it to the quad kernel on
    2048 workgroups, 32 products per lane, once ZK_LEAD_MIN_PAIRS / ZK_SKIP1_MIN_PAIRS keep the LEAD + SKIP1 k_round_kd (which comes
    first in launch_round) away from it.  Every round polynomial against the closed form -- the first round that differs is named -- and
    the challenges against pyref's verifier replaying the transcript."""
    import zk_amd
    from oracle import pyref
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd import ProductPoly, SumcheckProver

    field, n = zk_amd.BN254_FR, 24
    ctx = zk_amd.Context(field, 0)
    for name in ("const(O)", "const(M)"):
        tabs, closed = et.family(field, name, n, 2)
        a = MLE.new(ctx, n, tabs[0])
        s = closed.true_sum()
        proof, ch = SumcheckProver(2).prove_partial(ProductPoly.new([a, a]), et.elems(field, [s])[0])
        a.free()
        rp = [orc.to_ints(field, r) for r in proof.round_polys]
        want_rp = closed.round_polys(2, orc.to_ints(field, ch))
        for r in range(n):
            assert rp[r] == want_rp[r], ("round polynomial vs closed form", name, "round", r)
        sub, want_ch = pyref.sumcheck_verify_partial(field, s, rp)
        assert orc.to_ints(field, ch) == want_ch, ("challenges vs the replayed transcript", name)
        assert sub == closed.evaluate(want_ch), name
    print(f"extreme quad24 ok: 2 x {n} rounds (" + " ".join(f"{k}={os.environ.get(k)}" for k in
          ("ZK_QUAD_MAX_PAIRS", "ZK_PIPE_MAX_PAIRS", "ZK_LEAD_MIN_PAIRS", "ZK_SKIP1_MIN_PAIRS")) + ")")


def main():
    import zk_amd
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd import ProductPoly, SumcheckProver, gkr

    checked = 0
    fields = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)[:N_FIELDS]
    for field in fields:
        ctx = zk_amd.Context(field, 0)
        raw = et.raws(field)

        def upload(tabs, n):
            return ProductPoly.new([MLE.new(ctx, n, t) for t in tabs])   # one buffer per factor, equal tables included

        def closed_rp(closed, D, ch):
            return np.stack([et.elems(field, r) for r in closed.round_polys(D, orc.to_ints(field, ch))])

        for n in SIZES:
            for k, D in shapes(field, n):
                cases = [(name,) + oracle_cache.extreme_case(field, name, k, D, n) for name in et.FAMILIES]
                polys = []
                for name, tabs, closed, want in cases:
                    where = (field, name, k, D, n)
                    pp = upload(tabs, n)
                    polys.append(pp)
                    got = pp.round_sums(D)
                    assert np.array_equal(got, want["sums"]), ("round_sums vs oracle",) + where
                    if closed is not None:
                        assert np.array_equal(got, et.elems(field, closed.round_sums(D))), ("round_sums vs closed form",) + where
                        assert np.array_equal(want["s0"], et.elems(field, [closed.true_sum()])[0]), ("claimed sum",) + where
                    checked += 1
                    for consume in (False, True):
                        for w in ("0", "5"):   # a WRONG claimed sum too: SKIP1 / LEAD rounds derive sums from the previous round's claim
                            q = upload(tabs, n) if consume else pp
                            proof, ch = SumcheckProver(D).prove_partial(q, want["s" + w], consume=consume)
                            assert np.array_equal(proof.round_polys, want["rp" + w]), ("round polys vs oracle", consume, w) + where
                            assert np.array_equal(ch, want["ch" + w]), ("challenges vs oracle", consume, w) + where
                            if closed is not None:
                                assert np.array_equal(proof.round_polys, closed_rp(closed, D, ch)), ("round polys vs closed form", consume, w) + where
                            checked += 1
                    for q, t in zip(pp.polynomials, tabs):
                        assert np.array_equal(q.evaluation_slice(), t), ("inputs intact",) + where
                # batches of three: two different families and the first one again on the same handles
                for i, (name, tabs, closed, want) in enumerate(cases):
                    j = (i + 1) % len(cases)
                    got = SumcheckProver(D).prove_partial_batch([polys[i], polys[j], polys[i]], [want["s0"], cases[j][3]["s0"], want["s0"]])
                    for (proof, ch), w in zip(got, (want, cases[j][3], want)):
                        assert np.array_equal(proof.round_polys, w["rp0"]) and np.array_equal(ch, w["ch0"]), ("batch", field, name, cases[j][0], k, D, n)
                    checked += 1
                for pp in polys:
                    for q in pp.polynomials:
                        q.free()
            # the two-term GKR layer shape A.B + C against the big-int definition (oracle/gkr_ref.py through the cache: plain Python, computed
            # once on the parent's CPU-only workers), final evaluations included
            for which, names in enumerate(TERMS):
                tabs, s, want_rp, want_ch, want_fin = oracle_cache.extreme_terms_case(field, which, n)
                poly = gkr.SumOfProductsPoly([[MLE.new(ctx, n, t) for t in term] for term in tabs])
                rp, ch, fin = gkr.prove_partial_terms(poly, 2, s)
                assert np.array_equal(rp, want_rp), ("terms round polys", field, names, n)
                assert np.array_equal(ch, want_ch), ("terms challenges", field, names, n)
                assert np.array_equal(fin, want_fin), ("terms final evaluations", field, names, n)
                for q in poly.flat():
                    q.free()
                checked += 1
            # prod_reduce, and partial_evaluate at position 0 and one inner position with challenges of representation M, O, ONE, Z
            for name in et.FAMILIES:
                tabs, _ = et.family(field, name, n, 2, fill_random=orc.fill_random, seed=oracle_cache.EXTREME_SEED + 20)
                pp = upload(tabs, n)
                assert np.array_equal(pp.prod_reduce(), orc.prod_reduce(field, n, tabs)), ("prod_reduce", field, name, n)
                checked += 1
                for q, t in zip(pp.polynomials, tabs):
                    for pos in sorted({0, n // 2}):
                        for c in CHALLENGES:
                            asg = et.limbs(raw[c])[None, :]
                            folded = q.partial_evaluate(pos, asg)
                            got = folded.evaluation_slice()
                            folded.free()
                            assert np.array_equal(got, orc.mle_partial_evaluate(field, n, t, pos, asg)), ("partial_evaluate", field, name, n, pos, c)
                    q.free()
                checked += 1
    assert checked == expected_checks(SIZES, N_FIELDS), (checked, expected_checks(SIZES, N_FIELDS))
    switches = " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("ZK_") and k != "ZK_ORACLE_CACHE")
    print(f"extreme ok: {checked} checks ({switches})")


if __name__ == "__main__":
    {"eval": main_eval, "quad24": main_quad24}.get(sys.argv[1] if len(sys.argv) > 1 else "", main)()
