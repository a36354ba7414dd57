"""zk_merkle_commit / _root / _level / _open / zk_merkle_verify_host on the device.  The reference has no Merkle tree: tests/merkle_ref.py
is the definition.  One launch per level, fused stages over tiles of 2^3 and 2^10 and the default in child processes under ZK_MERKLE_FUSE_LEVELS,
every level byte for byte against the definition on every tree size and on the column counts at which the sponge can go wrong; in the
parent the wrapper on all three fields (root, a second commitment over stale pool blocks, untouched columns, batched openings with and
without rows, the host verifier on them), the error table, the measurement hook, one larger tree and the C++ mirror.  And the sizes at
which the kernels' loops take more than one trip (grids are capped at 2^19 threads and at 65536 tiles): trees of 2^20 and 2^21 rows in the
same child processes, level by level against the bulk reference; more opened items than the gather's grid has threads; a tree of 27
variables, whose levels lie past 4 GiB, in child processes of its own."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MerkleTree
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd._lib import c, lib, u8p, u64p

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merkle_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402
from merkle_check import FIELD_IDS, SETTINGS, SWITCH, TREE27_SETTINGS, digest, large_key  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "merkle_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BAD, ARITY, MISMATCH, UNSUP = -20, -4, -26, -25


@pytest.fixture(scope="module")
def child_lines():
    """{setting: the split lines of the child's output}: one child process per switch setting"""
    out = {}
    for setting, extra in SETTINGS.items():
        env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **extra)
        r = subprocess.run([sys.executable, CHECK, setting], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
        assert f"merkle {setting} ok" in r.stdout
        out[setting] = [ln.split() for ln in r.stdout.splitlines()]
    return out


@pytest.fixture(scope="module")
def children(child_lines):
    """{setting: {(field id, case): digest of all levels}}"""
    return {setting: {(ln[1], ln[2]): ln[3] for ln in lines if ln and ln[0] == "DIGEST"} for setting, lines in child_lines.items()}


@pytest.fixture(scope="module")
def large_children(child_lines):
    """{setting: {(field id, case, level): digest of that level}} of the large trees"""
    return {setting: {(ln[1], ln[2], int(ln[3])): ln[4] for ln in lines if ln and ln[0] == "LEVEL"} for setting, lines in child_lines.items()}


@pytest.fixture(scope="module")
def large_expected():
    """{(field id, case): [digest of level d for d in 0 .. n]} from the bulk reference, computed once (13 * 2^20 permutations on the
    oracle's threads)"""
    out = {}
    for fi, n, k, _ in ref.LARGE_CASES:
        _, images = ref.large_columns(FIELDS[fi], fi, n, k, worst_case_values)
        out[(FIELD_IDS[fi], large_key(n, k))] = [digest([lv]) for lv in ref.commit_bulk(images)]
    return out


@pytest.fixture(scope="module")
def expected():
    """{(field id, case): digest of all levels} from the definition, computed once"""
    out = {}
    for fi, field in enumerate(FIELDS):
        p = orc.modulus(field)
        for n, k in ref.CASES:
            levels = ref.commit(ref.columns_for(p, fi, n, k, worst_case_values))
            out[(FIELD_IDS[fi], f"n{n}_k{k}")] = digest([b"".join(lv) for lv in levels])
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_level_of_every_shape_on_every_path(children, expected, setting):
    """n = 0 .. 13 with one column and n in {0, 1, 3, 9, 10, 11} with 2, 4, 5, 17, 18, 34 and 35 columns, all three fields: the bytes of
    every level equal the definition's with one launch per level, with fused stages over tiles of 2^3 and of 2^10, and by default"""
    got = children[setting]
    assert len(expected) == 3 * len(ref.CASES) == 3 * 56 and set(got) == set(expected)
    wrong = sorted(key for key, want in expected.items() if got[key] != want)
    assert not wrong, (setting, wrong)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_level_of_the_trees_whose_loops_wrap(large_children, large_expected, setting):
    """n = 20, k = 1 on all three fields (k_merkle_leaves takes 2 trips of its grid-stride loop; with tiles of 2^3 k_merkle_fused takes 2
    tiles per workgroup) and n = 21, k = 1 on BN254 (k_merkle_level takes 2 trips, the leaves 4) on every path; n = 20, k = 5 on
    BLS12-377 (two-block leaves) level by level and with tiles of 2^10: every level's bytes equal the bulk reference's.  0, p - 1 and
    worst-case limb patterns sit on both sides of rows 2^19 and 2^20 and at the end."""
    got = large_children[setting]
    want = {(fid, case, d): dg for (fid, case), levels in large_expected.items() for d, dg in enumerate(levels)
            if any(setting in st and (FIELD_IDS[fi], large_key(n, k)) == (fid, case) for fi, n, k, st in ref.LARGE_CASES)}
    assert len(want) == sum(n + 1 for _, n, _, st in ref.LARGE_CASES if setting in st) >= 3 * 21 + 22
    assert set(got) == set(want)
    wrong = sorted(key for key, dg in want.items() if got[key] != dg)
    assert not wrong, (setting, wrong)


@pytest.mark.parametrize("setting", TREE27_SETTINGS)
def test_tree_of_27_variables(setting):
    """2^27 rows, one column, BN254, in a child process: with tiles of 2^10 it has 2^17 tiles on 65536 workgroups, the smallest tree at
    which that path takes a second tile, and level by level 256 trips of the leaves; every level above the leaves starts past 4 GiB of
    the tree's one block.  It cannot be referenced in full, so merkle_check.tree27 pins it through what is anchored already: (a) levels
    17 .. 27 and the root rebuilt by the definition from the downloaded level 16, (b) twelve slices of 2^16 rows (0, 7, 8, 1023, 1024,
    2047 and six seeded ones) committed on their own, whose roots must be their entries of level 16, (c) sixteen rows (0, 2^27 - 1, both
    sides of 2^19 and of 2^26, ten seeded) opened with their elements, accepted by merkle_ref.verify and by zk_amd.merkle_verify and
    rejected with one path byte flipped.  That pins the top, twelve whole 2^16-row sub-trees and sixteen root paths, not every byte."""
    env = dict({k: v for k, v in os.environ.items() if k != SWITCH}, **SETTINGS[setting])
    r = subprocess.run([sys.executable, CHECK, setting, "tree27"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"{setting} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert f"merkle {setting} tree27 ok" in r.stdout
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("TREE27")] == ["TREE27 top ok", "TREE27 slices ok", "TREE27 openings ok"]


@pytest.fixture(params=range(3), ids=FIELD_IDS)
def fctx(request):
    field = FIELDS[request.param]
    ctx = zk_amd.Context(field, 0)
    yield request.param, field, ctx
    ctx.close()


def _flip(b, byte, bit):
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


def _rejects(field, root, n, i, row, path):
    """the verifier says no, or refuses a row element that the flip pushed to p or above"""
    try:
        return not zk_amd.merkle_verify(field, root, n, i, row, path)
    except zk_amd.ZkError as e:
        return e.code == BAD


def test_commit_root_open_and_verify(fctx):
    fi, field, ctx = fctx
    p = orc.modulus(field)
    for n, k in ((0, 1), (0, 5), (1, 2), (4, 17), (11, 1), (11, 5)):
        ints = ref.columns_for(p, fi, n, k, worst_case_values)
        levels = ref.commit(ints)
        src = [orc.from_ints(field, col) for col in ints]
        cols = [MLE.new(ctx, n, s) for s in src]
        tree = MerkleTree.commit(cols)
        assert (tree.n_vars(), tree.n_columns()) == (n, k)
        assert tree.root() == ref.root(levels), (n, k)
        # a large non-zero table goes back to the pool: the blocks of the next commitment are cut from stale data, not zeros
        big = MLE.random(ctx, max(n + 1, 12), 77)
        MLE.random(ctx, n + 1, 78).free()
        big.free()
        again = MerkleTree.commit(cols)
        for d in range(n + 1):
            want = b"".join(levels[d])
            assert tree.level(d).tobytes() == want and again.level(d).tobytes() == want, (n, k, d)
        for s, col in zip(src, cols):
            assert np.array_equal(col.evaluation_slice(), s), (n, k, "a column changed")
        # batched openings: first and last row, both sides of the tile boundaries, a duplicate
        idx = ref.query_indices(n)
        rows, paths = tree.open(idx, cols)
        assert rows.shape == (len(idx), k, 4) and paths.shape == (len(idx), n, 32)
        for q, i in enumerate(idx):
            want_row, want_path = ref.open(levels, ints, i)
            assert orc.to_ints(field, rows[q]) == want_row, (n, k, i)
            assert paths[q].tobytes() == b"".join(want_path), (n, k, i)
            assert zk_amd.merkle_verify(field, tree.root(), n, i, rows[q], paths[q])
            bad_row = rows[q].copy()
            bad_row[q % k, 0] ^= np.uint64(2)
            assert _rejects(field, tree.root(), n, i, bad_row, paths[q])
            assert not zk_amd.merkle_verify(field, _flip(tree.root(), q, 3), n, i, rows[q], paths[q])
            if n:
                assert not zk_amd.merkle_verify(field, tree.root(), n, i, rows[q], _flip(paths[q].tobytes(), 32 * (q % n) + 5, 7))
                assert not zk_amd.merkle_verify(field, tree.root(), n, i ^ (1 << (q % n)), rows[q], paths[q])
        # without the columns: the same paths, no rows; the columns may be gone by then (the tree does not refer to them)
        for col in cols:
            col.free()
        MLE.random(ctx, n, 79).free()
        none_rows, only_paths = tree.open(idx)
        assert none_rows is None and np.array_equal(only_paths, paths)
        empty_rows, empty_paths = tree.open([])
        assert empty_rows is None and empty_paths.shape == (0, n, 32)
        assert again.root() == ref.root(levels)
        tree.free()
        again.free()


def test_error_table_and_bench_hook():
    field = zk_amd.BN254_FR
    ctx, other = zk_amd.Context(field, 0), zk_amd.Context(field, 0)
    a, b, small = MLE.random(ctx, 6, 1), MLE.random(ctx, 6, 2), MLE.random(ctx, 5, 3)
    a_other = MLE.random(other, 6, 1)
    before = a.evaluation_slice().copy()

    def arr(handles):
        hs = (c.c_void_p * len(handles))(*[None if t is None else t._h for t in handles])
        return c.cast(hs, c.POINTER(c.c_void_p)), hs

    h, ms = c.c_void_p(), c.c_double(-1.0)
    two, _k1 = arr([a, b])
    with_null, _k2 = arr([a, None])
    foreign, _k3 = arr([a, a_other])
    mixed, _k4 = arr([a, small])
    many, _k5 = arr([a] * 1025)
    many_mixed, _k6 = arr([a] * 1024 + [small])
    # commit: nulls and no columns, another context, mixed sizes, too many columns -- in this order
    assert lib.zk_merkle_commit(None, two, 2, c.byref(h)) == BAD
    assert lib.zk_merkle_commit(ctx._h, None, 2, c.byref(h)) == BAD
    assert lib.zk_merkle_commit(ctx._h, two, 2, None) == BAD
    assert lib.zk_merkle_commit(ctx._h, two, 0, c.byref(h)) == BAD
    assert lib.zk_merkle_commit(ctx._h, with_null, 2, c.byref(h)) == BAD
    assert lib.zk_merkle_commit(ctx._h, foreign, 2, c.byref(h)) == MISMATCH
    assert lib.zk_merkle_commit(other._h, two, 2, c.byref(h)) == MISMATCH
    assert lib.zk_merkle_commit(ctx._h, mixed, 2, c.byref(h)) == ARITY
    assert lib.zk_merkle_commit(ctx._h, many, 1025, c.byref(h)) == UNSUP
    assert lib.zk_merkle_commit(ctx._h, many_mixed, 1025, c.byref(h)) == ARITY   # the arity is looked at first
    assert not h.value
    assert lib.zk_bench_merkle(ctx._h, foreign, 2, 0, 1, c.byref(ms)) == MISMATCH
    assert lib.zk_bench_merkle(ctx._h, mixed, 2, 0, 1, c.byref(ms)) == ARITY
    assert lib.zk_bench_merkle(ctx._h, many, 1025, 0, 1, c.byref(ms)) == UNSUP
    assert lib.zk_bench_merkle(ctx._h, two, 2, 3, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_merkle(ctx._h, two, 2, 0, 0, c.byref(ms)) == BAD
    assert ms.value == -1.0
    # 1024 columns are fine (the pointer table takes 32 launches): the same column 1024 times
    wide, _k7 = arr([small] * 1024)
    assert lib.zk_merkle_commit(ctx._h, wide, 1024, c.byref(h)) == 0 and h.value
    wide_tree = MerkleTree(ctx, h)
    ints = orc.to_ints(field, small.evaluation_slice())
    assert wide_tree.root() == ref.root(ref.commit([ints] * 1024))
    wide_tree.free()
    # level, root, open on a real tree
    tree = MerkleTree.commit([a, b])
    buf = np.full(64 * 32, 7, dtype=np.uint8)
    bp = buf.ctypes.data_as(u8p)
    assert lib.zk_merkle_level(ctx._h, tree._h, 7, bp) == BAD                      # level > n
    assert lib.zk_merkle_level(other._h, tree._h, 0, bp) == MISMATCH
    assert lib.zk_merkle_root(other._h, tree._h, bp) == MISMATCH
    assert lib.zk_merkle_root(ctx._h, tree._h, None) == BAD
    idx = np.array([0, 64], dtype=np.uint64)
    rows = np.full((2, 2, 4), 7, dtype=np.uint64)
    ip, rp = idx.ctypes.data_as(u64p), rows.ctypes.data_as(u64p)
    assert lib.zk_merkle_open(ctx._h, tree._h, two, 2, ip, 2, rp, bp) == BAD       # index 64 >= 2^6
    assert lib.zk_merkle_open(ctx._h, tree._h, None, 0, ip, 2, None, bp) == BAD
    assert lib.zk_merkle_open(ctx._h, tree._h, two, 1, ip, 1, rp, bp) == BAD       # another number of columns
    assert lib.zk_merkle_open(ctx._h, tree._h, two, 2, None, 1, rp, bp) == BAD
    assert lib.zk_merkle_open(ctx._h, tree._h, two, 2, ip, 1, rp, None) == BAD
    assert lib.zk_merkle_open(ctx._h, tree._h, two, 2, ip, 1, None, bp) == BAD
    assert lib.zk_merkle_open(ctx._h, tree._h, with_null, 2, ip, 1, rp, bp) == BAD
    assert lib.zk_merkle_open(other._h, tree._h, two, 2, ip, 1, rp, bp) == MISMATCH
    assert lib.zk_merkle_open(ctx._h, tree._h, foreign, 2, ip, 1, rp, bp) == MISMATCH
    assert lib.zk_merkle_open(ctx._h, tree._h, mixed, 2, ip, 1, rp, bp) == ARITY
    assert (buf == 7).all() and (rows == 7).all()                                   # nothing was written by any of them
    assert lib.zk_merkle_open(ctx._h, tree._h, two, 2, None, 0, None, None) == 0    # no queries: a no-op
    # the measurement hook gives a time on every path and leaves the columns and the tree alone
    root = tree.root()
    for path in (0, 1, 2):
        ms.value = -1.0
        assert lib.zk_bench_merkle(ctx._h, two, 2, path, 2, c.byref(ms)) == 0 and ms.value > 0, path
        assert MerkleTree.bench([a, b], path=path, reps=1) > 0
    assert np.array_equal(a.evaluation_slice(), before) and tree.root() == root
    assert MerkleTree.commit([a, b]).root() == root
    ctx.close()
    other.close()


@pytest.fixture(scope="module")
def larger_tree():
    """n = 16, k = 2, BN254 on the default path, with the definition's levels (2^17 hashes on the C oracle), built once"""
    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    n = 16
    src = [orc.fill_random(field, 0x3E4 + j, 1 << n) for j in range(2)]
    ints = [orc.to_ints(field, s) for s in src]
    levels = ref.commit(ints)
    cols = [MLE.new(ctx, n, s) for s in src]
    tree = MerkleTree.commit(cols)
    yield field, n, src, ints, levels, cols, tree
    ctx.close()


def test_one_larger_tree_on_the_default_path(larger_tree):
    """n = 16, k = 2, BN254: the root and 64 seeded openings against the definition (2^17 hashes on the C oracle)"""
    field, n, src, ints, levels, cols, tree = larger_tree
    assert tree.root() == ref.root(levels)
    rng = random.Random(0x16)
    idx = [rng.randrange(1 << n) for _ in range(64)]
    rows, paths = tree.open(idx, cols)
    for q, i in enumerate(idx):
        want_row, want_path = ref.open(levels, ints, i)
        assert np.array_equal(rows[q], np.stack([src[0][i], src[1][i]])) and orc.to_ints(field, rows[q]) == want_row
        assert paths[q].tobytes() == b"".join(want_path), i
        assert zk_amd.merkle_verify(field, tree.root(), n, i, rows[q], paths[q])
    assert tree.level(8).tobytes() == b"".join(levels[8])


def test_more_opened_items_than_the_gather_has_threads(larger_tree):
    """2^15 + 3 seeded rows of the n = 16, k = 2 tree in one call, row 0, the last row and duplicates among them: 32,771 x (16 siblings +
    2 elements) = 589,878 items against the 2^19 = 524,288 threads of k_merkle_gather's capped grid, so its loop takes a second trip.
    Every row and every path against merkle_ref.open, taken for all queries at once from the definition's levels."""
    field, n, src, ints, levels, cols, tree = larger_tree
    rng = random.Random(0x6A7)
    idx = [0, (1 << n) - 1] + [rng.randrange(1 << n) for _ in range((1 << 15) - 1)]
    idx += [idx[5], idx[-1]]
    assert len(idx) == (1 << 15) + 3 and len(idx) * (n + 2) > 2048 * 256 and len(set(idx)) < len(idx)
    at = np.array(idx, dtype=np.uint64)
    level_arrays = [np.frombuffer(b"".join(lv), dtype=np.uint8).reshape(-1, 32) for lv in levels]
    want_paths = np.stack([level_arrays[d][(at >> np.uint64(d)) ^ np.uint64(1)] for d in range(n)], axis=1)
    want_rows = np.stack([s[at] for s in src], axis=1)
    for q in (0, 1, len(idx) - 1):   # the vectorised form is merkle_ref.open's
        want_row, want_path = ref.open(levels, ints, idx[q])
        assert orc.to_ints(field, want_rows[q]) == want_row and want_paths[q].tobytes() == b"".join(want_path)
    rows, paths = tree.open(idx, cols)
    assert rows.shape == want_rows.shape and paths.shape == want_paths.shape
    bad_rows = np.flatnonzero((rows != want_rows).any(axis=(1, 2)))
    bad_paths = np.flatnonzero((paths != want_paths).any(axis=(1, 2)))
    assert bad_rows.size == 0 and bad_paths.size == 0, (bad_rows[:8], bad_paths[:8], bad_rows.size, bad_paths.size)
    # without the rows: 32,771 x 16 items, one trip again
    none_rows, only_paths = tree.open(idx)
    assert none_rows is None and np.array_equal(only_paths, want_paths)


def test_openings_of_wide_rows_wrap_the_gather():
    """512 rows of a tree over 1024 columns (n = 5, the same column 1024 times, as the error-table test builds it): 512 x (5 + 1024) =
    526,848 items, more than the gather's grid has threads, nearly all of them row elements.  Every row and path against the definition."""
    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    n, k = 5, 1024
    small = MLE.random(ctx, n, 3)
    limbs = small.evaluation_slice()
    ints = orc.to_ints(field, limbs)
    levels = ref.commit([ints] * k)
    tree = MerkleTree.commit([small] * k)
    assert tree.root() == ref.root(levels)
    rng = random.Random(0x1024)
    idx = [0, 31, 31] + [rng.randrange(1 << n) for _ in range(509)]
    assert len(idx) * (n + k) > 2048 * 256
    rows, paths = tree.open(idx, [small] * k)
    assert rows.shape == (512, k, 4) and paths.shape == (512, n, 32)
    for q, i in enumerate(idx):
        want_row, want_path = ref.open(levels, [ints] * k, i)
        assert want_row == [ints[i]] * k
        assert np.array_equal(rows[q], np.broadcast_to(limbs[i], (k, 4))), (q, i)
        assert paths[q].tobytes() == b"".join(want_path), (q, i)
    ctx.close()


def test_cpp_host_mirror(tmp_path):
    """tests/cpp/test_merkle.cpp over zk.hpp: commit, root, levels, open and verify against the definition written out over zk_keccak256"""
    exe = str(tmp_path / "test_merkle")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_merkle.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: merkle host tests passed" in r.stdout
