"""bench.py --dump-outputs: the files it writes for a fold output of the timed shape (2^23 elements of 4 x u64 limbs) are
float64, fit in 64 MiB, hold the sampled elements exactly, cover every element through the digest, and come out the same
from run to run (CPU only: the helper is given a host array)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _fold_out():
    return np.random.default_rng(3).integers(0, 1 << 63, size=(1 << 23, 4), dtype=np.uint64)


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_files_exact_and_deterministic(tmp_path):
    a = _fold_out()
    r = np.array([1, 2, 3, (1 << 64) - 1], dtype=np.uint64)
    names = bench.dump_outputs(str(tmp_path / "x"), "", a, r)
    assert bench.dump_outputs(str(tmp_path / "y"), "", a, r) == names
    x, y = _load(tmp_path / "x"), _load(tmp_path / "y")
    assert sorted(x) == names == sorted(y)
    assert all(v.dtype == np.float64 for v in x.values())
    assert sum(v.nbytes for v in x.values()) <= 64 << 20
    for f in names:
        assert np.array_equal(x[f], y[f]), f
    idx = x["fold_out_sample_index.npy"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0)
    assert np.array_equal(x["fold_out_sample.npy"].astype(np.uint32).view(np.uint64), a[idx])
    assert np.array_equal(x["fold_challenge.npy"].astype(np.uint32).view(np.uint64), r)


def test_dump_outputs_digest_sees_every_element(tmp_path):
    a = _fold_out()
    names = bench.dump_outputs(str(tmp_path / "a"), "", a, np.zeros(4, dtype=np.uint64))
    idx = set(np.load(tmp_path / "a" / "fold_out_sample_index.npy").astype(np.int64).tolist())
    j = next(i for i in range(len(a)) if i not in idx)   # an element outside the sample
    b = a.copy()
    b[j, 2] ^= np.uint64(1)
    bench.dump_outputs(str(tmp_path / "b"), "", b, np.zeros(4, dtype=np.uint64))
    x, y = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert np.array_equal(x["fold_out_sample.npy"], y["fold_out_sample.npy"])
    assert not np.array_equal(x["fold_out_digest.npy"], y["fold_out_digest.npy"])
    # swapping two elements changes the digest too (position-weighted)
    c = a.copy()
    c[[j, j + 1]] = c[[j + 1, j]]
    bench.dump_outputs(str(tmp_path / "c"), "", c, np.zeros(4, dtype=np.uint64))
    assert not np.array_equal(x["fold_out_digest.npy"], np.load(tmp_path / "c" / "fold_out_digest.npy"))
    assert names == sorted(os.listdir(tmp_path / "c"))
