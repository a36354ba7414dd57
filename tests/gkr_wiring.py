"""Fan-in-2 layer wiring with PRESCRIBED CSR row lengths, for the GKR bookkeeping kernels (zk_amd/csrc/gkr_kernels.cuh).

Random wiring gives Poisson(1) rows, the one distribution k_gkr_phase was tuned for.  The kernels' row and chunk arithmetic depends
on how many gates read each input wire: a workgroup owns kGkrRows = 224 rows and walks their entries in chunks of kBlock = 256,
rows of more than kGkrHeavyRow = 256 entries leave the entry-parallel kernel for one workgroup each.  layer() builds a gate list in
which input wire i is the LEFT input of exactly left_lens[i] gates and the RIGHT input of exactly right_lens[i] gates; which gates
those are is a seeded random subset, so the eq gathers stay scattered.  Pure numpy: host and GPU tests share the named profiles.
"""
import numpy as np

ROWS, CHUNK, HEAVY = 224, 256, 256   # kGkrRows, kBlock, kGkrHeavyRow
OPS = ("random", "add", "mul")


def fill(special, rows, total, cap, seed=0):
    """row lengths: special = {row: length} as given, every other row a seeded draw of at most `cap` entries, sum exactly `total`"""
    lens = np.zeros(rows, dtype=np.int64)
    for r, n in special.items():
        lens[r] = n
    free = np.array([r for r in range(rows) if r not in special], dtype=np.int64)
    rem = total - int(lens.sum())
    assert 0 <= rem <= cap * len(free), f"{rem} gates do not fit {len(free)} rows of at most {cap}"
    rng = np.random.default_rng(seed)
    while rem:
        room = free[lens[free] < cap]
        lens += np.bincount(rng.choice(room, size=rem), minlength=rows)
        lens[free] = np.minimum(lens[free], cap)
        rem = total - int(lens.sum())
    return lens


def layer(log_out, log_in, left_lens, right_lens, ops="random", seed=0):
    """-> (log_out, log_in, op u8, left u32, right u32) with np.bincount(left) == left_lens and np.bincount(right) == right_lens"""
    n, rows = 1 << log_out, 1 << log_in
    rng = np.random.default_rng(seed)
    sides = []
    for lens in (left_lens, right_lens):
        lens = np.asarray(lens, dtype=np.int64)
        assert len(lens) == rows and int(lens.sum()) == n and lens.min() >= 0
        side = np.repeat(np.arange(rows, dtype=np.uint32), lens)
        sides.append(side[rng.permutation(n)])   # row i's gates: a random subset of the gate indices
    assert ops in OPS
    op = rng.integers(0, 2, n, dtype=np.uint8) if ops == "random" else np.full(n, OPS.index(ops) - 1, dtype=np.uint8)
    return log_out, log_in, op, sides[0], sides[1]


def random_layer(log_out, log_in, seed):
    """uniformly random wiring and ops"""
    rng = np.random.default_rng(seed)
    n = 1 << log_out
    return (log_out, log_in, rng.integers(0, 2, n, dtype=np.uint8), rng.integers(0, 1 << log_in, n, dtype=np.uint32),
            rng.integers(0, 1 << log_in, n, dtype=np.uint32))


# ---- the named profiles of a (log_out, log_in) = (12, 8) layer: 4096 gates over 256 rows, two workgroups of k_gkr_phase ---------------
P_OUT, P_IN = 12, 8
# Rows at both sides of the heavy/light boundary: first rows, a workgroup's last row (223), the next one's first (224), the last row.
# The seven special rows hold 1794 gates; the other 249 rows take the remaining 2302, which needs rows of up to 10.
THRESHOLD_SPECIAL = {0: 255, 1: 256, 2: 257, 3: 258, 223: 255, 224: 256, 255: 257}
THRESHOLD_CAP = 10
# Heavy rows with a light row of 200..256 entries directly before and after; every other row has at most 3 entries.
HBL_HEAVY = {1: 300, 100: 513, 223: 1024, 224: 257}
HBL_LIGHT = {0: 256, 2: 200, 99: 255, 101: 201, 222: 256, 225: 230}
HBL_CAP = 3


def _straddle():
    # 17 and 19 alternating on workgroup 0's rows: 4032 entries = 15.75 chunks, rows straddling every chunk boundary but one
    # (36 * 64 = 9 * 256: row 128 starts a chunk); the last 64 gates on workgroup 1's rows
    return np.array([17, 19] * (ROWS // 2) + [2] * 32)


def _tail_only():
    return np.array([0] * ROWS + [128] * 32)   # workgroup 0: e_lo == e_hi, no chunk at all


def profile_lens(name):
    """-> (left_lens, right_lens) of a named profile; the right profile is the left one reversed unless stated otherwise"""
    n, rows = 1 << P_OUT, 1 << P_IN
    if name == "threshold":
        left = fill(THRESHOLD_SPECIAL, rows, n, THRESHOLD_CAP, seed=1)
    elif name == "straddle":
        left = _straddle()
    elif name == "aligned":
        left = np.full(rows, 16)   # every chunk ends exactly on a row boundary
    elif name == "tail_only":
        left = _tail_only()
    elif name == "head_only":
        left = _tail_only()[::-1]   # rows 224..255 empty: workgroup 1 has no chunk
    elif name == "heavy_between_light":
        left = fill({**HBL_HEAVY, **HBL_LIGHT}, rows, n, HBL_CAP, seed=2)
    elif name == "one_left_row":
        left = np.zeros(rows, dtype=np.int64)
        left[77] = n
        return left, np.full(rows, 16)
    elif name.endswith("_mirrored"):   # the two sides swapped: the RIGHT CSR (phase 2) gets the rows placed at 223 / 224 / 255
        left, right = profile_lens(name[:-len("_mirrored")])
        return right, left
    else:
        raise ValueError(name)
    return np.asarray(left, dtype=np.int64), np.asarray(left, dtype=np.int64)[::-1].copy()


PROFILES = ("threshold", "straddle", "aligned", "tail_only", "head_only", "heavy_between_light", "one_left_row", "threshold_mirrored",
            "heavy_between_light_mirrored")
# (profile, ops): every profile with random ops; the two with heavy rows also all-add and all-mul (the op bit masks the parked addends)
CASES = tuple((name, "random") for name in PROFILES) + tuple((name, ops) for name in ("threshold", "heavy_between_light") for ops in ("add", "mul"))
# rows of more than HEAVY entries each side of a profile must have: (left, right)
N_HEAVY = {"threshold": (3, 3), "straddle": (0, 0), "aligned": (0, 0), "tail_only": (0, 0), "head_only": (0, 0),
           "heavy_between_light": (4, 4), "one_left_row": (1, 0), "threshold_mirrored": (3, 3), "heavy_between_light_mirrored": (4, 4)}


def profile_layer(name, ops="random"):
    left, right = profile_lens(name)
    return layer(P_OUT, P_IN, left, right, ops, seed=1000 + PROFILES.index(name))


# ---- a large skewed layer: heavy rows, rows at the boundary and long light rows packed into the same workgroups ------------------------
SKEW_OUT, SKEW_IN = 19, 18
SKEW_DENSE_ROWS = 1 << 14
N_UNIFORM = 800   # rows drawn from 200..256 (at most 204800 gates: with the rows below they fit the 2^19 gates of the layer)


def skewed_special(seed):
    """the multiset of special row lengths, in a seeded order"""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[70001, 1025], np.full(300, 256), np.full(300, 257), np.full(300, 255), rng.integers(200, 257, N_UNIFORM)])
    return lens.astype(np.int64)


def skewed_lens(seed, order_seed):
    """The special rows sit on a seeded subset of the first SKEW_DENSE_ROWS rows (some 23 of them, over 5000 entries, in every
    workgroup there: twenty chunks next to heavy rows); the remaining gates are spread at random over all the other rows."""
    n, rows = 1 << SKEW_OUT, 1 << SKEW_IN
    special = skewed_special(seed)
    rng = np.random.default_rng(order_seed)
    at = rng.choice(SKEW_DENSE_ROWS, size=len(special), replace=False)
    lens = np.zeros(rows, dtype=np.int64)
    lens[at] = rng.permutation(special)
    free = np.setdiff1d(np.arange(rows), at)
    rem = n - int(lens.sum())
    assert rem >= 0
    lens += np.bincount(rng.choice(free, size=rem), minlength=rows)
    return lens


def skewed_layer(seed=7):
    return layer(SKEW_OUT, SKEW_IN, skewed_lens(seed, seed + 1), skewed_lens(seed, seed + 2), "random", seed=seed + 3)
