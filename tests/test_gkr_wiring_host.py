"""CPU checks of tests/gkr_wiring.py (wiring with prescribed CSR row lengths) and, on its shapes, of the checker the GPU tests rest on:
tests/gkr_oracle_check.py must accept the big-int model's proof of a (12 -> 8) profile layer and reject a corrupted one, as
tests/test_gkr_model.py shows for random wiring."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gkr_wiring as gw  # noqa: E402


@pytest.mark.parametrize("name,ops", gw.CASES)
def test_profile_rows_have_the_requested_lengths(name, ops):
    want_l, want_r = gw.profile_lens(name)
    log_out, log_in, op, left, right = gw.profile_layer(name, ops)
    n, rows = 1 << log_out, 1 << log_in
    assert (log_out, log_in) == (gw.P_OUT, gw.P_IN)
    assert op.dtype == np.uint8 and left.dtype == np.uint32 and right.dtype == np.uint32
    assert op.shape == left.shape == right.shape == (n,)
    assert np.array_equal(np.bincount(left, minlength=rows), want_l)
    assert np.array_equal(np.bincount(right, minlength=rows), want_r)
    assert (int((want_l > gw.HEAVY).sum()), int((want_r > gw.HEAVY).sum())) == gw.N_HEAVY[name]
    if name != "one_left_row":
        assert np.array_equal(want_r, want_l[::-1])
    if ops == "random":
        assert 0 < int(op.sum()) < n
        # a row's gates are scattered over the gate list, not a run of consecutive indices
        long_rows = np.flatnonzero(want_l >= 16)
        z = np.flatnonzero(left == long_rows[0])
        assert z.max() - z.min() >= 4 * len(z) or len(z) == n
    else:
        assert np.all(op == (ops == "mul"))


def test_profiles_are_what_their_names_say():
    rows = 1 << gw.P_IN
    thr, _ = gw.profile_lens("threshold")
    assert [int(thr[i]) for i in (0, 1, 2, 3, 223, 224, 255)] == [255, 256, 257, 258, 255, 256, 257]
    others = np.delete(thr, list(gw.THRESHOLD_SPECIAL))
    assert others.max() <= gw.THRESHOLD_CAP and others.sum() == 4096 - 1794
    st, _ = gw.profile_lens("straddle")
    assert list(st[:gw.ROWS]) == [17, 19] * 112 and st[:gw.ROWS].sum() == 4032 and st[gw.ROWS:].sum() == 64
    ends = np.cumsum(st[:gw.ROWS])[:-1]   # row boundaries inside workgroup 0: one is chunk-aligned, 222 are not
    assert list(ends[ends % gw.CHUNK == 0]) == [2304]
    al, _ = gw.profile_lens("aligned")
    assert np.all(np.cumsum(al) % 16 == 0) and np.all(al == 16)
    tail, tail_r = gw.profile_lens("tail_only")
    head, head_r = gw.profile_lens("head_only")
    assert tail[:gw.ROWS].sum() == 0 and np.all(tail[gw.ROWS:] == 128)
    assert head[gw.ROWS:].sum() == 0 and head.sum() == 4096 and np.array_equal(head, tail_r) and np.array_equal(head_r, tail)
    hbl, _ = gw.profile_lens("heavy_between_light")
    for r, n in gw.HBL_HEAVY.items():
        assert hbl[r] == n > gw.HEAVY
        for nb in (r - 1, r + 1):
            assert nb in gw.HBL_HEAVY or 200 <= hbl[nb] <= gw.HEAVY
    assert np.delete(hbl, list(gw.HBL_HEAVY) + list(gw.HBL_LIGHT)).max() <= gw.HBL_CAP
    one, one_r = gw.profile_lens("one_left_row")
    assert one[77] == 4096 and np.count_nonzero(one) == 1 and np.all(one_r == 16) and len(one) == rows


def test_fill_and_layer_reject_impossible_requests():
    assert gw.fill({0: 5}, 4, 11, 2).tolist()[0] == 5 and gw.fill({0: 5}, 4, 11, 2).sum() == 11
    assert gw.fill({}, 8, 0, 3).sum() == 0
    with pytest.raises(AssertionError):
        gw.fill({0: 5}, 4, 12, 2)
    with pytest.raises(AssertionError):
        gw.layer(2, 1, [3, 2], [2, 2])
    with pytest.raises(AssertionError):
        gw.layer(2, 1, [2, 2, 0], [2, 2])


def test_skewed_layer_has_the_special_rows_on_both_sides():
    log_out, log_in, op, left, right = gw.skewed_layer()
    assert (log_out, log_in) == (gw.SKEW_OUT, gw.SKEW_IN)
    special = np.sort(gw.skewed_special(7))
    assert special[-1] == 70001 and special[-2] == 1025
    for side in (left, right):
        lens = np.bincount(side, minlength=1 << log_in)
        assert lens.sum() == 1 << log_out
        assert np.array_equal(np.sort(lens[lens >= 200]), special)   # the same multiset on both sides
        assert (lens > gw.HEAVY).sum() == 302 and (lens == 256).sum() >= 300 and (lens == 255).sum() >= 300
        wg = np.add.reduceat(lens[:gw.ROWS * 64], np.arange(0, gw.ROWS * 64, gw.ROWS))   # entries per workgroup of the dense part
        assert wg.min() > 4 * gw.CHUNK
    assert not np.array_equal(np.bincount(left, minlength=1 << log_in), np.bincount(right, minlength=1 << log_in))


@pytest.mark.parametrize("name,ops", [("threshold", "random"), ("heavy_between_light", "add"), ("tail_only", "random")])
def test_oracle_checker_agrees_with_the_model_on_profile_layers(name, ops):
    """check_proof (C oracle primitives only) accepts gkr_ref.gkr_prove's proof of the depth-1 circuit [(12 -> 8 profile)] and rejects it
    with one element changed (the model's own verifier is not run here: test_gkr_model.py pins it to the model's prover)"""
    from oracle import binding as orc
    from oracle import gkr_ref
    from tests.gkr_oracle_check import check_proof

    field = 1
    p = orc.modulus(field)
    L = gw.profile_layer(name, ops)
    layers = [(L[0], L[1], L[2].tolist(), L[3].tolist(), L[4].tolist())]
    rng = random.Random(41)
    ins = [rng.randrange(p) for _ in range(1 << gw.P_IN)]
    seed = bytes(rng.randrange(256) for _ in range(32))
    outs, proof = gkr_ref.gkr_prove(field, layers, ins, seed)
    assert len(proof) == 6 * gw.P_IN + 2
    F =lambda xs: orc.from_ints(field, xs)  # noqa: E731
    ok, why = check_proof(field, [L], F(ins), F(outs), seed, F(proof))
    assert ok, why
    for pos in (0, len(proof) // 2, len(proof) - 1):
        bad = list(proof)
        bad[pos] = (bad[pos] + 1) % p
        assert not check_proof(field, [L], F(ins), F(outs), seed, F(bad))[0], f"corrupted proof element {pos} accepted"
