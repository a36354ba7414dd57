"""What tests/test_gpu_pcs_large.py rests on, checked without a GPU: the identity that lets a big quotient be compared with two of half
its size, the oracle-transform LDE against the definition's, the sample set, and the arithmetic by which each shape of tests/pcs_ref.py
reaches the loop trip it is there for (so that a later change of a constant breaks loudly).  Everything is Python integers."""
import os
import random
import sys

import pytest

from oracle import binding as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_ref  # noqa: E402
import pcs_ref as ref  # noqa: E402
from divrem_check import LARGE  # noqa: E402


@pytest.mark.parametrize("field", range(3), ids=fri_ref.FIELD_IDS)
def test_even_and_odd_outputs_are_the_quotients_of_the_even_and_odd_rows(field):
    """quotient(cols, s)[0::2] == quotient(even rows, s) and [1::2] == quotient(odd rows, s w_N), with the same z, values and alpha:
    x_{2i} = s (w_N^2)^i and x_{2i+1} = (s w_N) (w_N^2)^i, and w_N^2 is the root of the half-size domain"""
    p = fri_ref.modulus(field)
    rng = random.Random(0xE0DD + field)
    for log_n in range(1, 7):
        w = fri_ref.root(field, 1 << log_n)
        for k in (1, 3):
            cols = [[rng.randrange(p) for _ in range(1 << log_n)] for _ in range(k)]
            ys, alpha = [rng.randrange(p) for _ in range(k)], rng.randrange(p)
            for s in (1, 5, p - 1, rng.randrange(1, p)):
                z = rng.randrange(p)
                while ref.on_domain(field, log_n, s, z):
                    z = rng.randrange(p)
                whole = ref.quotient(field, cols, s, z, ys, alpha)
                assert whole[0::2] == ref.quotient(field, [col[0::2] for col in cols], s, z, ys, alpha), (log_n, k, s)
                assert whole[1::2] == ref.quotient(field, [col[1::2] for col in cols], s * w % p, z, ys, alpha), (log_n, k, s)
                assert all(whole[i] == ref.quotient_at(field, lambda c, j: cols[c][j], k, log_n, s, z, ys, alpha, i) for i in range(1 << log_n))


@pytest.mark.parametrize("field", range(3), ids=fri_ref.FIELD_IDS)
def test_the_oracle_transform_lde_is_the_definitions(field):
    p = fri_ref.modulus(field)
    rng = random.Random(0x1DE0 + field)
    for log_n in range(0, 9):
        for length in sorted({1, (1 << log_n) // 2, (1 << log_n) - 1, 1 << log_n} - {0}):
            coeffs = [rng.randrange(p) for _ in range(length)]
            coeffs[-1] = p - 1
            for shift in (1, 5, p - 1):
                got = ref.lde_by_oracle(field, coeffs, log_n, shift)
                assert got.shape == (1 << log_n, 4) and orc.to_ints(field, got) == fri_ref.lde(field, coeffs, log_n, shift), (log_n, length, shift)


@pytest.mark.parametrize("log_n", sorted({lg - h for lg, _ in ref.BIG_QUOTIENTS for h in (0, 1)}))   # the big quotients and their halves
def test_the_samples_of_a_big_quotient(log_n):
    n, per = 1 << log_n, ref.totals_per_thread(log_n)
    for count in (ref.BIG_SAMPLES, ref.BIG_HALF_SAMPLES):
        idx = ref.quotient_big_samples(log_n, count)
        assert len(idx) == count and len(set(idx)) == count and idx == sorted(idx) and 0 <= idx[0] and idx[-1] < n
        assert {0, n - 1, 63, 64, 2047, 2048, 4095, 4096} <= set(idx)
        for t in (1, 2, 128, 255, 256):   # thread t of k_pcs_totals starts at chunk t per; 256 per chunks is the whole table
            assert {b for b in (2048 * per * t - 1, 2048 * per * t) if b < n} <= set(idx), t
        assert 2048 * per * 256 == n and idx == ref.quotient_big_samples(log_n, count)   # seeded: the same set in parent and child
    assert len(ref.quotient_big_samples(log_n)) == 4096


def test_each_shape_reaches_the_trip_it_is_there_for():
    # a second batch of column pointers from 33 columns on; the widest commitment is the limit itself
    assert ref.PTR_BATCH == 32 and min(ref.WIDE_QUOTIENT_COLUMNS) == ref.PTR_BATCH and 33 in ref.WIDE_QUOTIENT_COLUMNS and 65 in ref.WIDE_QUOTIENT_COLUMNS
    assert all((case[0] << case[3]) > 2 * ref.PTR_BATCH for _, case in ref.WIDE_CASES)
    assert ref.WIDE_MAX_CASE[0] << ref.WIDE_MAX_CASE[3] == ref.MAX_COLUMNS == ref.WIDE_QUOTIENT_MAX[1] == 1024
    # the trace gather: 513 queries of 1024 row elements and one sibling pass the 2^19 threads of the capped grid by 1,537 items (512
    # queries are the first that do, by 512: 512 x 1025 = 524,800; up to 511 one sweep covers them)
    assert 513 * 1025 > 512 * 1025 > 1 << 19 >= 511 * 1025
    assert ref.GATHER_THREADS == 1 << 19 and ref.gather_items(ref.WIDE_MAX_CASE) == 513 * 1025 == 525825
    assert all(ref.gather_items(case) <= ref.GATHER_THREADS for case in ref.CASES + ref.GPU_EXTRA_CASES)   # none of the earlier cases wraps
    # partial sums per polynomial of the evaluation
    assert [ref.eval_partials(d) for d in (12, 13, 14, 15, 19)] == [1, 2, 4, 8, 64]
    assert max(case[1] for case in ref.GPU_CASES) == 12 and [case[1] for _, case in ref.MID_CASES] == [13, 14, 15]
    assert (1 << 19) // 16 > 64 * 256 and ref.BIG_CASE[1] == 19   # more runs of 16 coefficients than threads: the loop's second trip
    # chunk products per thread of k_pcs_totals: one up to 2^19 points (every thread busy exactly there), 2 and 4 at the big sizes
    assert ref.totals_per_thread(max(ref.QUOTIENT_LOGS)) == 1 and ref.totals_per_thread(19) == 1 and (1 << 19) // ref.CHUNK == ref.TOTALS_THREADS
    assert [ref.totals_per_thread(lg) for lg, _ in ref.BIG_QUOTIENTS] == [2, 4]
    assert ref.totals_per_thread(ref.BIG_CASE[1] + ref.BIG_CASE[2]) == 2   # the big opening's quotient, through zk_pcs_open
    # the edge sizes are new, and the launch they take: below 64 points no wave runs, up to 2^11 one workgroup alone
    assert not set(ref.EDGE_QUOTIENT_LOGS) & set(ref.QUOTIENT_LOGS)
    assert 1 << 5 < 64 <= 1 << 6 and 1 << 9 <= ref.CHUNK < 1 << 12
    # the linear division's middle launch: 258 chunks of 4096 coefficients on 256 threads, two per thread, a ragged top chunk
    la = (1 << 20) + 4097
    assert (la, 2, (0,)) in LARGE["linear"] and -(-la // 4096) == 258 and -(-258 // 256) == 2 and la % 4096 == 1
    assert max(-(-a // 4096) for a, lb, _ in LARGE["linear"] + LARGE["model"] if lb == 2 and a != la) <= 256
