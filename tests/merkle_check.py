"""Run by tests/test_gpu_merkle.py in child processes (the library reads its ZK_* switches once per process), and imported by it for
the settings, so that the parent and the children hold the same cases.

  python merkle_check.py <setting>    setting: default | levels | fuse3 | fuse10
      under ZK_MERKLE_FUSE_LEVELS as the parent sets it: per field and case (n, k) of tests/merkle_ref.py a digest of every level of
      zk_merkle_commit's tree (zk_merkle_level for level 0 .. n, concatenated); then, per large case of merkle_ref.LARGE_CASES that
      names this setting, one digest per level (LEVEL lines: a mismatch names the level)
  python merkle_check.py <setting> tree27
      the tree of 27 variables (tree27 below); exits non-zero on the first check that does not hold"""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import merkle_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from merkle_ref import CASES, columns_for  # noqa: E402

FIELD_IDS = ("bn254", "bls12_381", "bls12_377")
SWITCH = "ZK_MERKLE_FUSE_LEVELS"
# levels: one launch per level; fuse3: tiles of 2^3, so that trees of 7 to 13 variables take several fused stages and the one-workgroup
# top; fuse10: the largest tile, four leaves per thread and more nodes than threads on the first level of the climb from 10 variables on;
# default: what ships
SETTINGS = {"default": {}, "levels": {SWITCH: "0"}, "fuse3": {SWITCH: "3"}, "fuse10": {SWITCH: "10"}}
# the tree of 27 variables: on fuse10 2^17 tiles on 65536 workgroups (the smallest tree at which that path takes a second tile), on
# levels 256 trips of the leaves; one block of 8 GiB in which every level above the leaves starts past 4 GiB
TREE27_SETTINGS = ("levels", "fuse10")
TREE27_VARS, TREE27_SLICE_VARS, TREE27_SEED = 27, 16, 0x27EE
TREE27_SLICES = (0, 7, 8, 1023, 1024, 2047)      # 8 and 1024: the first rows of the second leaf trip and of the second tile trip
TREE27_ROWS = (0, (1 << 27) - 1, (1 << 19) - 1, 1 << 19, (1 << 26) - 1, 1 << 26)


def digest(levels_bytes):
    return hashlib.sha256(b"".join(levels_bytes)).hexdigest()


def large_key(n, k):
    return f"n{n}_k{k}"


def check(setting):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MerkleTree
    from zk_amd import MultiLinearPolynomial as MLE

    assert os.environ.get(SWITCH) == SETTINGS[setting].get(SWITCH), os.environ.get(SWITCH)
    fields = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)
    for fi, field in enumerate(fields):
        ctx = zk_amd.Context(field, 0)
        p = orc.modulus(field)
        for n_vars in (0, 1, 4, 8, 10, 12, 14):   # stale pool data in the size classes of the trees
            MLE.random(ctx, n_vars, 900 + n_vars).free()
        for n, k in CASES:
            cols = [MLE.new(ctx, n, orc.from_ints(field, col)) for col in columns_for(p, fi, n, k, worst_case_values)]
            tree = MerkleTree.commit(cols)
            assert tree.n_vars() == n and tree.n_columns() == k
            print("DIGEST", FIELD_IDS[fi], f"n{n}_k{k}", digest([tree.level(d).tobytes() for d in range(n + 1)]))
            tree.free()
        ctx.close()
    for fi, n, k, settings in ref.LARGE_CASES:
        if setting not in settings:
            continue
        ctx = zk_amd.Context(fields[fi], 0)
        MLE.random(ctx, n + 1, 950 + n).free()   # the tree's block is cut from stale data, not zeros
        limbs, _ = ref.large_columns(fields[fi], fi, n, k, worst_case_values)
        cols = [MLE.new(ctx, n, a) for a in limbs]
        tree = MerkleTree.commit(cols)
        for d in range(n + 1):
            print("LEVEL", FIELD_IDS[fi], large_key(n, k), d, digest([tree.level(d).tobytes()]))
        tree.free()
        ctx.close()
    print(f"merkle {setting} ok")


def tree27(setting):
    """One tree of 27 variables, one column, BN254, the library's own generator.  It cannot be referenced in full, so it is pinned
    through what is anchored already: (a) levels 17 .. 27 rebuilt by the definition from the downloaded level 16; (b) twelve slices of
    2^16 rows committed on their own (a tree of 16 variables, on the same path, which does not wrap there), whose roots must be the
    entries of level 16; (c) sixteen rows opened and verified by the definition and by the host verifier.  That pins the top, twelve
    whole 2^16-row sub-trees and sixteen root paths, not every byte."""
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MerkleTree
    from zk_amd import MultiLinearPolynomial as MLE

    assert os.environ.get(SWITCH) == SETTINGS[setting].get(SWITCH), os.environ.get(SWITCH)
    field = zk_amd.BN254_FR
    n, sub_n = TREE27_VARS, TREE27_SLICE_VARS
    top = n - sub_n
    ctx = zk_amd.Context(field, 0)
    table = MLE.random(ctx, n, TREE27_SEED)
    tree = MerkleTree.commit([table])
    assert (tree.n_vars(), tree.n_columns()) == (n, 1)
    # (a) the top of the tree from level 16
    anchor = tree.level(sub_n)
    rebuilt = ref.climb(anchor.tobytes())
    assert len(rebuilt) == top + 1
    for d in range(sub_n + 1, n + 1):
        assert tree.level(d).tobytes() == rebuilt[d - sub_n], ("level", d)
    root = tree.root()
    assert root == rebuilt[-1], "root"
    print("TREE27 top ok")
    # (b) rows [j 2^16, (j + 1) 2^16) as a table of their own: variable 0 is the most significant index bit
    rng = random.Random(0x27)
    slices = list(TREE27_SLICES)
    while len(slices) < len(TREE27_SLICES) + 6:
        j = rng.randrange(1 << top)
        if j not in slices:
            slices.append(j)
    for j in slices:
        bits = orc.from_ints(field, [(j >> (top - 1 - t)) & 1 for t in range(top)])
        part = table.partial_evaluate(0, bits)
        assert part.n_vars() == sub_n
        sub = MerkleTree.commit([part])
        assert sub.root() == anchor[j].tobytes(), ("slice", j)
        sub.free()
        part.free()
    print("TREE27 slices ok")
    # (c) openings with rows
    idx = list(TREE27_ROWS) + [rng.randrange(1 << n) for _ in range(10)]
    rows, paths = tree.open(idx, [table])
    for q, i in enumerate(idx):
        row = orc.to_ints(field, rows[q])
        path = [paths[q, d].tobytes() for d in range(n)]
        assert ref.verify(root, n, 1, i, row, path), ("definition", i)
        assert zk_amd.merkle_verify(field, root, n, i, rows[q], paths[q]), ("host verifier", i)
        flipped = bytearray(paths[q].tobytes())
        flipped[32 * (q % n) + q] ^= 1 << (q % 8)
        assert not ref.verify(root, n, 1, i, row, [bytes(flipped[32 * d:32 * d + 32]) for d in range(n)]), ("definition, flipped", i)
        assert not zk_amd.merkle_verify(field, root, n, i, rows[q], bytes(flipped)), ("host verifier, flipped", i)
    print("TREE27 openings ok")
    tree.free()
    table.free()
    ctx.close()
    print(f"merkle {setting} tree27 ok")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "tree27":
        tree27(sys.argv[1])
    else:
        check(sys.argv[1])
