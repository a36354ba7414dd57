"""The definition of the library's batch inversion and running products (zk_mle_batch_inverse, zk_upoly_batch_inverse,
zk_mle_prefix_product, zk_batch_inverse_host; the reference has neither), in plain Python integers, and the cases the host and GPU
tests share.  A field inverse is unique, so every correct algorithm gives the bits of pow(x, p - 2, p): no tolerance anywhere."""
import random

# the kernel's chunk (zk_amd/csrc/inv_kernels.cuh: kInvChunk = kBlock * kInvPerThread) and workgroup size; thread t of a chunk owns the
# elements base + q * BLOCK + t.  tests/test_batch_inverse_host.py checks them against the source, so that the boundary sizes below keep
# pointing at the real boundaries when the kernel is retuned.
BLOCK = 256
CHUNK = 2048
PER_THREAD = CHUNK // BLOCK
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
LOG_CHUNK = CHUNK.bit_length() - 1
MLE_VARS = (0, 1, 6, LOG_CHUNK - 1, LOG_CHUNK, LOG_CHUNK + 1)


def batch_inverse(vals, shift, p, cache=None):
    """([(v + shift)^-1 mod p, 0 where v + shift == 0], number of zeros).  `cache` only remembers pow results between calls."""
    out, zeros = [], 0
    for v in vals:
        x = (v + shift) % p
        if x == 0:
            zeros += 1
            out.append(0)
            continue
        inv = cache.get(x) if cache is not None else None
        if inv is None:
            inv = pow(x, p - 2, p)
            if cache is not None:
                cache[x] = inv
        out.append(inv)
    return out, zeros


def prefix_product(vals, inclusive, p):
    """exclusive: out[0] = 1, out[i] = vals[0] ... vals[i-1]; inclusive: out[i] = vals[0] ... vals[i]; and the product of all"""
    out, acc = [], 1 % p
    for v in vals:
        if not inclusive:
            out.append(acc)
        acc = acc * v % p
        if inclusive:
            out.append(acc)
    return out, acc


def base_values(p, field_index, n, worst_case_values):
    """n canonical values without a zero: random ones with the structured worst-case Montgomery limbs (tests/field_corpus.py) spread
    over the front, so that every length from a few elements on holds some"""
    rng = random.Random(0xB1A5 + 977 * field_index + n)
    vals = [rng.randrange(1, p) for _ in range(n)]
    worst = [w for w in worst_case_values(p, field_index, min(n, 512)) if w] + [p - 1, 1]   # (the last ones win a shared slot)
    for k, w in enumerate(worst):
        vals[(k * 7) % n] = w
    return vals


def zero_placements(n, chunk=CHUNK, block=BLOCK):
    """{name: sorted indices < n that hold a zero}.  Thread t of chunk c owns c * chunk + q * block + t, q < chunk / block: its
    first element is q = 0, its last q = chunk / block - 1."""
    last_q = chunk // block - 1
    t = 5 % block   # some thread that is not the first of its wave
    clip = lambda idx: sorted({i for i in idx if 0 <= i < n})  # noqa: E731
    last_chunk = (n - 1) // chunk * chunk if n else 0
    return {
        "zero_at_0": clip([0]),
        "zero_at_last": clip([n - 1]),
        "group_first_and_last": clip([t, last_q * block + t, last_chunk + t, last_chunk + last_q * block + t]),
        "chunk_first_and_last": clip([0, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk]),
        "whole_group": clip([last_chunk + q * block + t for q in range(last_q + 1)]),
        "whole_chunk": clip(range(last_chunk, last_chunk + chunk)),
        "all_zero": clip(range(n)),
        "two_adjacent": clip([n // 2, n // 2 + 1]),
    }


def cases(p, field_index, n, worst_case_values):
    """[(name, values, shift)]: the random values with and without a shift, every zero placement (no shift), and a zero that only
    the shift produces (the table itself has none)"""
    rng = random.Random(0x5F17 + field_index)
    shift = rng.randrange(1, p)
    base = base_values(p, field_index, n, worst_case_values) if n else []
    out = [("random", base, 0), ("random_shift", base, shift)]
    for name, idx in zero_placements(n).items():
        v = list(base)
        for i in idx:
            v[i] = 0
        out.append((name, v, 0))
    target = p - shift   # in [1, p): t[i] = target is not zero, t[i] + shift is
    v = [x if x != target else (2 if target == 1 else 1) for x in base]
    for i in zero_placements(n)["chunk_first_and_last"] + zero_placements(n)["two_adjacent"]:
        v[i] = target
    out.append(("zero_by_shift_only", v, shift))
    return out
