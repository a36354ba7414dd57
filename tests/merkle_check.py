"""Run by tests/test_gpu_merkle.py in child processes (the library reads its ZK_* switches once per process), and imported by it for
the settings, so that the parent and the children hold the same cases.

  python merkle_check.py <setting>    setting: default | levels | fuse3 | fuse10
      under ZK_MERKLE_FUSE_LEVELS as the parent sets it: per field and case (n, k) of tests/merkle_ref.py a digest of every level of
      zk_merkle_commit's tree (zk_merkle_level for level 0 .. n, concatenated)"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from field_corpus import worst_case_values  # noqa: E402
from merkle_ref import CASES, columns_for  # noqa: E402

FIELD_IDS = ("bn254", "bls12_381", "bls12_377")
SWITCH = "ZK_MERKLE_FUSE_LEVELS"
# levels: one launch per level; fuse3: tiles of 2^3, so that trees of 7 to 13 variables take several fused stages and the one-workgroup
# top; fuse10: the largest tile, four leaves per thread and more nodes than threads on the first level of the climb from 10 variables on;
# default: what ships
SETTINGS = {"default": {}, "levels": {SWITCH: "0"}, "fuse3": {SWITCH: "3"}, "fuse10": {SWITCH: "10"}}


def digest(levels_bytes):
    return hashlib.sha256(b"".join(levels_bytes)).hexdigest()


def check(setting):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MerkleTree
    from zk_amd import MultiLinearPolynomial as MLE

    assert os.environ.get(SWITCH) == SETTINGS[setting].get(SWITCH), os.environ.get(SWITCH)
    for fi, field in enumerate((zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)):
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
    print(f"merkle {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
