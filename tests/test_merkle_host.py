"""The definition of the Merkle commitments (tests/merkle_ref.py) checked on its own, the host verifier zk_merkle_verify_host against it on
all three fields, its error table, the pinned root of the one-zero-element tree, the new exports and their Python signatures -- all
without a GPU."""
import ctypes as c
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from oracle import pyref
from zk_amd import ZkError, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merkle_ref as ref  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
BAD, BAD_FIELD, UNSUP = -20, -21, -25
SYMBOLS = ("zk_merkle_commit", "zk_merkle_free", "zk_merkle_n_vars", "zk_merkle_n_columns", "zk_merkle_root", "zk_merkle_level", "zk_merkle_open",
           "zk_merkle_verify_host", "zk_bench_merkle")


def _no_gpu():
    n = c.c_int32()
    _lib.lib.zk_device_count(c.byref(n))
    return n.value == 0


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _verify_raw(field, root, n, k, index, row_limbs, path_bytes):
    """(status, ok) of zk_merkle_verify_host on raw buffers"""
    ok = c.c_int32(-7)
    rt, pv = _u8(root), _u8(path_bytes)
    rc = _lib.lib.zk_merkle_verify_host(field, rt.ctypes.data_as(_lib.u8p), n, k, index, row_limbs.ctypes.data_as(_lib.u64p),
                                        pv.ctypes.data_as(_lib.u8p) if n else None, c.byref(ok))
    return rc, ok.value


def test_exports_signatures_and_abi_version():
    assert _lib.lib.zk_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    assert "#define ZK_AMD_ABI_VERSION 6" in header
    for name in SYMBOLS:
        assert hasattr(_lib.lib, name), name
        assert name in _lib._sig and name in _lib.declared_symbols(), name
        assert re.search(r"\bint32_t %s\(" % name, header), name
    assert "MerkleTree" in zk_amd.api.__all__ and "merkle_verify" in zk_amd.api.__all__
    assert hasattr(zk_amd, "MerkleTree") and hasattr(zk_amd, "merkle_verify")


def test_definition_is_self_consistent():
    p = orc.modulus(0)
    a, b = 5, p - 1
    levels = ref.commit([[a, b]])
    assert ref.root(levels) == orc.keccak256(orc.keccak256(a.to_bytes(32, "big")) + orc.keccak256(b.to_bytes(32, "big")))
    # two columns: the leaf is the hash of the concatenated row
    levels = ref.commit([[a, b], [7, 9]])
    assert levels[0][1] == orc.keccak256(b.to_bytes(32, "big") + (9).to_bytes(32, "big"))
    for n, k in ((0, 1), (0, 3), (1, 2), (3, 5), (5, 17)):
        cols = ref.columns_for(p, 0, n, k, worst_case_values)
        levels = ref.commit(cols)
        assert [len(lv) for lv in levels] == [1 << (n - d) for d in range(n + 1)]
        for i in range(1 << n):
            row, path = ref.open(levels, cols, i)
            assert len(path) == n and ref.verify(ref.root(levels), n, k, i, row, path)
            if n:
                assert not ref.verify(ref.root(levels), n, k, i ^ 1, row, path)
                assert not ref.verify(ref.root(levels), n, k, i, row, path[::-1]) or n == 1
    assert ref.CASES[:14] == tuple((n, 1) for n in range(14)) and len(ref.CASES) == 14 + 6 * 7
    assert ref.query_indices(11) == [0, 2047, 7, 8, 1023, 1024, 1024] and ref.query_indices(0) == [0, 0, 0]


def test_keccak256_many_is_keccak256_per_item():
    """the oracle's bulk hash against its one-item call at the lengths around the rate (136) and the two the trees use (32 k, 64), on
    more items than the oracle has threads; no items and empty items included"""
    rng = random.Random(0x3A27)
    for item_len in (0, 1, 32, 64, 135, 136, 137, 160):
        for count in (0, 1, 2, 67):
            data = bytes(rng.randrange(256) for _ in range(item_len * count))
            want = b"".join(orc.keccak256(data[item_len * i:item_len * (i + 1)]) for i in range(count))
            assert orc.keccak256_many(data, item_len, count) == want, (item_len, count)
            if item_len:
                assert orc.keccak256_many(np.frombuffer(data, dtype=np.uint8), item_len) == want, (item_len, count)
    assert orc.keccak256_many(b"", 0, 3) == 3 * pyref.keccak256(b"")


def test_commit_bulk_is_commit():
    """the bulk reference of the large trees against the definition on every shared case (BLS12-377), and large_columns' own promises
    on a small tree: the planted rows, the images, no two equal adjacent rows in column 0"""
    fi = 2
    p = orc.modulus(FIELDS[fi])
    for n, k in ref.CASES:
        cols = ref.columns_for(p, fi, n, k, worst_case_values)
        levels = ref.commit(cols)
        bulk = ref.commit_bulk([ref.be32_images(col) for col in cols])
        assert bulk == [b"".join(lv) for lv in levels], (n, k)
        # the images as the large trees take them: Montgomery limbs through the oracle's to_bytes
        via_oracle = [np.frombuffer(orc.mle_to_bytes(FIELDS[fi], n, orc.from_ints(FIELDS[fi], col)), dtype=np.uint8).reshape(1 << n, 32) for col in cols]
        assert all(np.array_equal(a, ref.be32_images(col)) for a, col in zip(via_oracle, cols)), (n, k)
    # the reference of the large trees: 32 k // 136 + 1 permutations per leaf and one per node
    assert sum((32 * k // 136 + 2) << n for _, n, k, _ in ref.LARGE_CASES) == 13 << 20
    assert all(set(settings) <= set(ref.LARGE_SETTINGS) for _, _, _, settings in ref.LARGE_CASES)
    n, k = 3, 2
    limbs, images = ref.large_columns(FIELDS[fi], fi, n, k, worst_case_values)
    assert len(limbs) == len(images) == k and all(a.shape == (8, 4) for a in limbs) and all(a.shape == (8, 32) for a in images)
    ints = [orc.to_ints(FIELDS[fi], a) for a in limbs]
    assert ints[0][-1] == p - 1 and ints[1][-1] == 0 and len(set(ints[0])) == 8
    assert ref.commit_bulk(images) == [b"".join(lv) for lv in ref.commit(ints)]


def test_pinned_root_of_the_one_zero_element_tree():
    """one column, n = 0, element 0: the root is keccak256 of 32 zero bytes, by the independent pure-Python Keccak"""
    want = bytes.fromhex("290decd9548b62a8d60345a988386fc84ba6bc95484008f6362f93160ef3e563")
    assert pyref.keccak256(bytes(32)) == want
    assert ref.root(ref.commit([[0]])) == want
    for field in FIELDS:
        assert zk_amd.merkle_verify(field, want, 0, 0, orc.from_ints(field, [0]), b"")
        assert not zk_amd.merkle_verify(field, want, 0, 0, orc.from_ints(field, [1]), b"")


@pytest.mark.parametrize("fi", range(3), ids=("bn254", "bls12_381", "bls12_377"))
def test_verify_host_against_the_definition(fi):
    """n in 0..6, k in {1, 4, 5, 17, 18}: every row's opening made by the definition is accepted; one flipped bit in the row, in each path
    digest, in the root or in the index is rejected, and so is a path with the right digests in the wrong order"""
    field = FIELDS[fi]
    p = orc.modulus(field)
    for n in range(7):
        for k in (1, 4, 5, 17, 18):
            cols = ref.columns_for(p, fi, n, k, worst_case_values)
            assert cols[0][0] == 0 or (n == 0 and k == 1)
            assert cols[-1][-1] == p - 1
            levels = ref.commit(cols)
            root = ref.root(levels)
            limbs = [orc.from_ints(field, col) for col in cols]   # Montgomery limbs, as they cross the ABI
            for i in range(1 << n):
                row, path = ref.open(levels, cols, i)
                rl = np.stack([limbs[j][i] for j in range(k)])
                pb = b"".join(path)
                assert _verify_raw(field, root, n, k, i, rl, pb) == (0, 1), (n, k, i)
                if i not in (0, (1 << n) - 1, (1 << n) // 2):
                    continue   # the rejections on the first, the middle and the last row
                bad = rl.copy()
                bad[(i + k // 2) % k, (i + n) % 4] ^= np.uint64(1 << ((7 * i + n) % 16))   # a low bit: the element stays below p or is refused
                rc, ok = _verify_raw(field, root, n, k, i, bad, pb)
                assert (rc, ok) == (0, 0) or rc == BAD, (n, k, i, "row")
                for d in range(n):
                    flipped = bytearray(pb)
                    flipped[32 * d + (i + d) % 32] ^= 1 << (d % 8)
                    assert _verify_raw(field, root, n, k, i, rl, flipped) == (0, 0), (n, k, i, d)
                flipped = bytearray(root)
                flipped[(i + k) % 32] ^= 0x80
                assert _verify_raw(field, flipped, n, k, i, rl, pb) == (0, 0), (n, k, i, "root")
                for d in range(n):
                    assert _verify_raw(field, root, n, k, i ^ (1 << d), rl, pb) == (0, 0), (n, k, i, d, "index")
                if n >= 2:
                    swapped = path[1] + path[0] + b"".join(path[2:])
                    assert _verify_raw(field, root, n, k, i, rl, swapped) == (0, 0), (n, k, i, "order")
                    assert _verify_raw(field, root, n, k, i, rl, b"".join(path[::-1])) == (0, 0), (n, k, i, "reversed")
            # the Python wrapper on the same opening
            row, path = ref.open(levels, cols, (1 << n) - 1)
            assert zk_amd.merkle_verify(field, root, n, (1 << n) - 1, orc.from_ints(field, row), b"".join(path))


def test_verify_host_error_table():
    lib = _lib.lib
    field = zk_amd.BN254_FR
    p = orc.modulus(field)
    cols = [[3, 4, 5, 6]]
    levels = ref.commit(cols)
    root = _u8(ref.root(levels))
    row, path = ref.open(levels, cols, 2)
    rl = orc.from_ints(field, row)
    pv = _u8(b"".join(path))
    ok = c.c_int32(-7)
    rp, pp, lp = root.ctypes.data_as(_lib.u8p), pv.ctypes.data_as(_lib.u8p), rl.ctypes.data_as(_lib.u64p)
    assert lib.zk_merkle_verify_host(field, rp, 2, 1, 2, lp, pp, c.byref(ok)) == 0 and ok.value == 1
    ok.value = -7
    assert lib.zk_merkle_verify_host(9, rp, 2, 1, 2, lp, pp, c.byref(ok)) == BAD_FIELD
    assert lib.zk_merkle_verify_host(field, None, 2, 1, 2, lp, pp, c.byref(ok)) == BAD
    assert lib.zk_merkle_verify_host(field, rp, 2, 1, 2, None, pp, c.byref(ok)) == BAD
    assert lib.zk_merkle_verify_host(field, rp, 2, 1, 2, lp, None, c.byref(ok)) == BAD
    assert lib.zk_merkle_verify_host(field, rp, 2, 1, 2, lp, pp, None) == BAD
    assert lib.zk_merkle_verify_host(field, rp, 2, 0, 2, lp, pp, c.byref(ok)) == BAD          # no columns
    assert lib.zk_merkle_verify_host(field, rp, 2, 1025, 2, lp, pp, c.byref(ok)) == UNSUP      # before the row is read
    assert lib.zk_merkle_verify_host(field, rp, 2, 1, 4, lp, pp, c.byref(ok)) == BAD          # index >= 2^n
    assert lib.zk_merkle_verify_host(field, rp, 0, 1, 1, lp, None, c.byref(ok)) == BAD
    # an element that is not fully reduced: the modulus itself and all ones, as zk_fe_from_canonical refuses them
    for v in (p, (1 << 256) - 1):
        raw = np.frombuffer(v.to_bytes(32, "little"), dtype="<u8").astype(np.uint64).reshape(1, 4)
        assert lib.zk_merkle_verify_host(field, rp, 2, 1, 2, raw.ctypes.data_as(_lib.u64p), pp, c.byref(ok)) == BAD
        assert lib.zk_fe_from_canonical(field, raw.ctypes.data_as(_lib.u64p), np.zeros(4, dtype=np.uint64).ctypes.data_as(_lib.u64p)) == BAD
    assert ok.value == -7   # nothing was written by any of them
    # p - 1 as limbs is fully reduced: a verdict, not an error
    raw = np.frombuffer((p - 1).to_bytes(32, "little"), dtype="<u8").astype(np.uint64).reshape(1, 4)
    assert lib.zk_merkle_verify_host(field, rp, 2, 1, 2, raw.ctypes.data_as(_lib.u64p), pp, c.byref(ok)) == 0 and ok.value == 0
    # the wrapper refuses a path of the wrong length before the call
    with pytest.raises(ZkError):
        zk_amd.merkle_verify(field, bytes(root), 2, 2, rl, b"".join(path)[:-1])


def test_device_calls_reject_null_arguments_without_gpu():
    lib = _lib.lib
    fake = c.c_void_p(8)   # never dereferenced: a NULL among the others ends the call first
    h, u, ms = c.c_void_p(), c.c_uint32(77), c.c_double(-1.0)
    one = (c.c_void_p * 1)(None)
    cols = c.cast(one, c.POINTER(c.c_void_p))
    buf = np.zeros(32, dtype=np.uint8)
    bp = buf.ctypes.data_as(_lib.u8p)
    assert lib.zk_merkle_commit(None, cols, 1, c.byref(h)) == BAD
    assert lib.zk_merkle_commit(fake, None, 1, c.byref(h)) == BAD
    assert lib.zk_merkle_commit(fake, cols, 0, c.byref(h)) == BAD
    assert lib.zk_merkle_commit(fake, cols, 1, c.byref(h)) == BAD      # a NULL column
    assert lib.zk_merkle_commit(fake, cols, 1, None) == BAD
    assert h.value is None
    assert lib.zk_merkle_free(None) == 0
    assert lib.zk_merkle_n_vars(None, c.byref(u)) == BAD and lib.zk_merkle_n_columns(None, c.byref(u)) == BAD
    assert lib.zk_merkle_n_vars(fake, None) == BAD and lib.zk_merkle_n_columns(fake, None) == BAD
    assert lib.zk_merkle_root(fake, None, bp) == BAD
    assert lib.zk_merkle_level(None, fake, 0, bp) == BAD and lib.zk_merkle_level(fake, None, 0, bp) == BAD
    assert lib.zk_merkle_level(fake, fake, 0, None) == BAD
    assert lib.zk_merkle_open(None, fake, None, 0, None, 0, None, None) == BAD
    assert lib.zk_merkle_open(fake, None, None, 0, None, 0, None, None) == BAD
    assert lib.zk_bench_merkle(None, cols, 1, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_merkle(fake, None, 1, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_merkle(fake, cols, 0, 0, 1, c.byref(ms)) == BAD
    assert lib.zk_bench_merkle(fake, cols, 1, 0, 1, None) == BAD
    assert lib.zk_bench_merkle(fake, cols, 1, 0, 0, c.byref(ms)) == BAD     # reps < 1
    assert lib.zk_bench_merkle(fake, cols, 1, 3, 1, c.byref(ms)) == BAD     # no such path
    assert lib.zk_bench_merkle(fake, cols, 1, -1, 1, c.byref(ms)) == BAD
    assert u.value == 77 and ms.value == -1.0 and not buf.any()


def test_switch_and_tile_constants_match_the_kernel_source():
    src = open(os.path.join(ROOT, "zk_amd", "csrc", "merkle_kernels.cuh")).read()
    host = open(os.path.join(ROOT, "zk_amd", "csrc", "merkle.hip")).read()
    header = open(os.path.join(ROOT, "include", "zk_amd.h")).read()
    tile = int(re.search(r"constexpr uint32_t kMerkleMaxTileLog = (\d+);", src).group(1))
    top = int(re.search(r"constexpr uint32_t kMerkleTopLog = (\d+);", src).group(1))
    default = int(re.search(r"constexpr uint32_t kMerkleFuseDefault = (\d+);", host).group(1))
    assert re.search(r'env_u64\("ZK_MERKLE_FUSE_LEVELS", kMerkleFuseDefault, 0, kMerkleMaxTileLog\)', host)
    assert re.search(r"ZK_MERKLE_FUSE_LEVELS\s+%d\s+0 \.\. %d\b" % (default, tile), header)   # the switch's default and range
    assert int(re.search(r"constexpr uint32_t kMerkleMaxColumns = (\d+);", src).group(1)) == 1024
    # the rows the GPU test opens straddle the tile boundaries of the forced setting (3) and of the largest tile
    assert ref.query_indices(tile + 1)[2:6] == [7, 8, (1 << tile) - 1, 1 << tile] and top == 6


def test_large_cases_sit_where_the_launch_code_caps_its_grids():
    """what tests/merkle_ref.py says of its large cases, from the launch code: grid_for gives at most kMaxGrid workgroups of 256 threads
    (2^19: the leaves wrap from 2^20 rows, a level from 2^20 nodes), the fused build at most kMerkleMaxGrid workgroups (tiles of 2^3 wrap
    from n = 20, tiles of 2^10 from n = 27)"""
    core = open(os.path.join(ROOT, "zk_amd", "csrc", "host_core.hpp")).read()
    host = open(os.path.join(ROOT, "zk_amd", "csrc", "merkle.hip")).read()
    threads = int(re.search(r"constexpr uint32_t kMaxGrid = (\d+);", core).group(1)) * 256
    tiles = int(re.search(r"constexpr uint32_t kMerkleMaxGrid = (\d+);", host).group(1))
    assert "if (b > kMaxGrid) b = kMaxGrid;" in core and "tiles < kMerkleMaxGrid ? tiles : kMerkleMaxGrid" in host
    assert (threads, tiles) == (1 << 19, 1 << 16) and ref.TRIP_BOUNDARIES == (threads, 2 * threads)
    assert min(n for _, n, _, _ in ref.LARGE_CASES) == 20 and 1 << 20 >= 2 * threads               # the leaves of every large case
    assert any(n == 21 for _, n, _, _ in ref.LARGE_CASES) and 1 << (21 - 1) >= 2 * threads         # level 1 of the n = 21 tree
    assert 1 << (20 - 3) == 2 * tiles and 1 << (27 - 10) == 2 * tiles                              # fuse3 at n = 20, fuse10 at n = 27
    import merkle_check

    assert merkle_check.TREE27_VARS == 27 and set(merkle_check.TREE27_SETTINGS) == {"levels", "fuse10"}
    assert merkle_check.TREE27_SLICES == (0, 7, 8, 1023, 1024, 2047)
    # slice 8: row 2^19, the first of the second leaf trip; slice 1024: row 2^26, the first of the second tile trip (65536 tiles of 2^10)
    assert 8 << merkle_check.TREE27_SLICE_VARS == threads and 1024 << merkle_check.TREE27_SLICE_VARS == tiles << 10
    assert (32771 * (16 + 2) > threads) and (512 * (5 + 1024) > threads)                           # the two gather tests


def test_commit_without_gpu_fails_loudly():
    if not _no_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ZkError) as e:
        ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
        zk_amd.MerkleTree.commit([zk_amd.MultiLinearPolynomial.new(ctx, 1, np.zeros((2, 4), dtype=np.uint64))])
    assert e.value.code == -22   # ZK_ERR_NO_DEVICE


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "test_merkle")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_merkle.cpp"),
                    "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, text=True)
    if not _no_gpu():
        pytest.skip("GPU present: run by tests/test_gpu_merkle.py")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr
