"""The definition of the library's Merkle commitments over tables (zk_merkle_commit, zk_merkle_root, zk_merkle_level, zk_merkle_open,
zk_merkle_verify_host; the reference has no Merkle tree, so this file is the definition), over plain Python integers and the C oracle's
Keccak-256 (oracle.binding.keccak256: original Keccak padding 0x01 ... 0x80, rate 136, the function of zk_keccak256), and the cases
the host and GPU tests share.  Everything is bytes: no tolerance anywhere.

  input    k >= 1 columns, each 2^n canonical integers (n >= 0), one field
  leaf     leaf[i] = Keccak256(be32(c_0[i]) || be32(c_1[i]) || ... || be32(c_{k-1}[i])), be32 = the 32-byte big-endian integer (the
           per-element image of MultiLinearPolynomial::to_bytes, evaluation_form.rs:97-103)
  node     level[d+1][j] = Keccak256(level[d][2j] || level[d][2j+1]), level[0] = leaf; root = level[n][0] (n = 0: the one leaf)
  opening  of row i: the row (c_0[i], ..., c_{k-1}[i]) and the path [level[d][(i >> d) ^ 1] for d in 0..n), bottom up
  verify   the leaf from the row, then per d: Keccak256(h || path[d]) if bit d of i is 0, Keccak256(path[d] || h) otherwise; == root

There are no domain-separation bytes: n and k are part of the statement and verify takes both, so a node is never read as a leaf."""
import random

import numpy as np

from oracle import binding as orc
from oracle.binding import keccak256, keccak256_many

# the shapes the GPU test commits to: every n with one column, and the column counts at which the sponge can go wrong (4: both padding
# bits in word 16; 5: the first element that straddles a block; 17: exactly four blocks, the padding a block of its own; 18: one element
# past the 17-element period; 34: two periods; 35: one element into the third) on trees below, at and above the fused tile sizes
SINGLE_COLUMN_VARS = tuple(range(14))
MULTI_COLUMN_VARS = (0, 1, 3, 9, 10, 11)
MULTI_COLUMN_COUNTS = (2, 4, 5, 17, 18, 34, 35)
CASES = tuple((n, 1) for n in SINGLE_COLUMN_VARS) + tuple((n, k) for n in MULTI_COLUMN_VARS for k in MULTI_COLUMN_COUNTS)


def be32(v):
    return int(v).to_bytes(32, "big")


def leaf(row):
    return keccak256(b"".join(be32(v) for v in row))


def commit(columns):
    """columns: k lists of 2^n canonical ints -> levels: levels[d] = the 2^(n - d) digests of level d"""
    rows = len(columns[0])
    assert columns and rows & (rows - 1) == 0 and rows >= 1 and all(len(col) == rows for col in columns)
    levels = [[leaf([col[i] for col in columns]) for i in range(rows)]]
    while len(levels[-1]) > 1:
        cur = levels[-1]
        levels.append([keccak256(cur[2 * j] + cur[2 * j + 1]) for j in range(len(cur) // 2)])
    return levels


def commit_bulk(be32_columns):
    """`commit` for trees too large to hash call by call: k arrays of shape (rows, 32), the big-endian images of the columns' elements
    -> the levels as bytes, level d = the 2^(n - d) digests concatenated.  `commit` stays the definition (tests/test_merkle_host.py
    holds the two equal on every shared case); this one makes one oracle call per level."""
    cols = [np.ascontiguousarray(col, dtype=np.uint8) for col in be32_columns]
    rows = cols[0].shape[0]
    assert cols and rows >= 1 and rows & (rows - 1) == 0 and all(col.shape == (rows, 32) for col in cols)
    return climb(keccak256_many(np.concatenate(cols, axis=1), 32 * len(cols), rows))


def climb(level):
    """the bytes of one level -> that level and every level above it, up to the root"""
    levels = [bytes(level)]
    while len(levels[-1]) > 32:
        levels.append(keccak256_many(levels[-1], 64))
    return levels


def be32_images(ints):
    """canonical ints -> the (len, 32) uint8 array commit_bulk takes"""
    return np.frombuffer(b"".join(be32(v) for v in ints), dtype=np.uint8).reshape(len(ints), 32)


def root(levels):
    return levels[-1][0]


def open(levels, columns, i):
    """(row, path) of row i"""
    n = len(levels) - 1
    return [col[i] for col in columns], [levels[d][(i >> d) ^ 1] for d in range(n)]


def verify(root_, n, k, i, row, path):
    if len(row) != k or len(path) != n or not 0 <= i < (1 << n):
        return False
    h = leaf(row)
    for d in range(n):
        h = keccak256(h + path[d]) if (i >> d) & 1 == 0 else keccak256(path[d] + h)
    return h == root_


def columns_for(p, field_index, n, k, worst_case_values):
    """k columns of 2^n canonical ints: seeded random values mixed with the worst-case limb patterns of tests/field_corpus.py, plus 0 and
    p - 1 (row 0 starts with 0, the last row ends with p - 1)"""
    rng = random.Random(0x3E4C1E + 1000 * field_index + 64 * n + k)
    rows = 1 << n
    worst = worst_case_values(p, field_index, 256) + [0, p - 1]
    cols = [[rng.choice(worst) if rng.random() < 0.25 else rng.randrange(p) for _ in range(rows)] for _ in range(k)]
    cols[0][0] = 0
    cols[-1][-1] = p - 1
    # no two rows alike (column 0 is made of distinct values): two equal sibling leaves would make an opening hold at either index
    last_fixed = k == 1   # then column 0 ends with the planted p - 1
    seen = {0, p - 1} if last_fixed else {0}
    for i in range(1, rows - 1 if last_fixed else rows):
        while cols[0][i] in seen:
            cols[0][i] = rng.randrange(p)
        seen.add(cols[0][i])
    return cols


# The trees at which the grid-stride loops take more than one trip (merkle.hip: grid_for caps k_merkle_leaves and k_merkle_level at
# 2048 workgroups of 256 threads = 2^19, the fused build at 65536 tiles): (field index, n, k, settings of tests/merkle_check.py).
#   n = 20, k = 1   leaves: 2 trips; fuse3: 2^17 tiles on 65536 workgroups, 2 tiles each
#   n = 21, k = 1   k_merkle_level: 2 trips on level 1 (2^20 nodes); leaves: 4
#   n = 20, k = 5   a two-block leaf with the element that straddles the blocks, inside a wrapped trip
LARGE_SETTINGS = ("default", "levels", "fuse3", "fuse10")
LARGE_CASES = ((0, 20, 1, LARGE_SETTINGS), (1, 20, 1, LARGE_SETTINGS), (2, 20, 1, LARGE_SETTINGS), (0, 21, 1, LARGE_SETTINGS),
               (2, 20, 5, ("levels", "fuse10")))
TRIP_BOUNDARIES = (1 << 19, 1 << 20)


def large_columns(field, field_index, n, k, worst_case_values):
    """(limbs, images) of the k columns of a large tree: limbs[j] the (2^n, 4) Montgomery elements as they are uploaded, images[j] their
    (2^n, 32) big-endian images by the oracle's own conversion.  The oracle's generator, with 0, p - 1 and worst-case limb patterns
    planted in the two rows on either side of every trip boundary and in the last two rows; column 0 has no two equal adjacent rows."""
    p, rows = orc.modulus(field), 1 << n
    worst = worst_case_values(p, field_index, 16)
    limbs = []
    for j in range(k):
        col = orc.fill_random(field, 0x3E4C1E00 + 4096 * field_index + 64 * n + j, rows)
        planted = {}
        for t, b in enumerate(TRIP_BOUNDARIES):
            edge = (0, p - 1) if (t + j) % 2 == 0 else (p - 1, 0)
            planted.update({b - 2: worst[(4 * t + j) % 16], b - 1: edge[0], b: edge[1], b + 1: worst[(4 * t + j + 1) % 16]})
        planted.update({rows - 2: worst[(8 + j) % 16], rows - 1: p - 1 if j % 2 == 0 else 0})
        at = sorted(r for r in planted if 0 <= r < rows)
        col[at] = orc.from_ints(field, [planted[r] for r in at])
        limbs.append(col)
    assert (limbs[0][1:] != limbs[0][:-1]).any(axis=1).all(), "column 0 has two equal adjacent rows"
    images = [np.frombuffer(orc.mle_to_bytes(field, n, col), dtype=np.uint8).reshape(rows, 32) for col in limbs]
    return limbs, images


def query_indices(n, tile_logs=(3, 10)):
    """the rows the GPU test opens: 0, 2^n - 1, both sides of every fused tile boundary that the tree has, and a duplicate"""
    last = (1 << n) - 1
    idx = [0, last]
    for s in tile_logs:
        if n > s:
            idx += [(1 << s) - 1, 1 << s]
    return idx + [idx[-1]]
