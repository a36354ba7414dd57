"""Merkle commitments on the device: the build of the whole tree (zk_bench_merkle: HIP events on the context's stream, the average of
--inner back-to-back builds after as many untimed ones) with the fused sub-tree stages and with one launch per level, BN254, one and
four columns, at 2^16, 2^20 and 2^24 rows; --samples such measurements per line: median and minimum, the two paths alternating.  Beside
each: zk_bench_copy of the bytes a commitment must move (k * 2^n * 32 read, (2^(n+1) - 1) * 32 written) from the same process as the
ceiling for bytes, and the Keccak-f[1600] permutations per second that the time implies (4k / 17 + 1 per leaf, one per node).  Then the
wall clock of zk_merkle_open for 64 rows with their elements at the largest size.  The tile of the fused path is the library's chosen
one unless ZK_MERKLE_FUSE_LEVELS is set for the run (read once per process); the setting is logged.
Output: profiles/merkle.log (--append adds a run, e.g. one with another tile, to the log).

  python tools/merkle_bench.py [--samples 5] [--max-log 24] [--append] [--out profiles/merkle.log]"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MerkleTree  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402

FIELD = zk_amd.BN254_FR
FUSED, LEVELS = 1, 2
NAMES = {FUSED: "fused stages", LEVELS: "level by level"}


def inner_reps(n_vars):
    return 10 if n_vars <= 16 else 3 if n_vars <= 20 else 1


def measure(cols, samples):
    """{path: (median ms, min ms)}; the paths alternate sample by sample"""
    n_vars = cols[0].n_vars()
    got = {p: [] for p in NAMES}
    for p in NAMES:
        MerkleTree.bench(cols, p, 1)   # warm: code objects, pool blocks
    for _ in range(samples):
        for p in NAMES:
            got[p].append(MerkleTree.bench(cols, p, inner_reps(n_vars)))
    return {p: (statistics.median(v), min(v)) for p, v in got.items()}


def block_builds(ctx, samples, max_log):
    lines = []
    for n_vars in (16, 20, 24):
        if n_vars > max_log:
            continue
        rows = 1 << n_vars
        for k in (1, 4):
            cols = [MLE.random(ctx, n_vars, 21 + j) for j in range(k)]
            r = measure(cols, samples)
            nbytes = 32 * (k * rows + 2 * rows - 1)
            gbps = statistics.median(ctx.bench_copy(max(nbytes // 2, 16), 5) for _ in range(3))   # the hook moves `bytes` in and `bytes` out
            copy_ms = nbytes / (gbps * 1e9) * 1e3
            perms = rows * (4 * k // 17 + 1) + rows - 1
            for p in NAMES:
                med, lo = r[p]
                lines.append(f"n=2^{n_vars:<2} k={k} {NAMES[p]:<15} median {med:9.4f} ms  min {lo:9.4f} ms  {perms / (med * 1e-3) / 1e9:7.3f} Gperm/s"
                             f"  | copy of the same {nbytes / 2**20:9.1f} MiB {copy_ms:8.4f} ms ({gbps / 1e3:.2f} TB/s): {copy_ms / med:6.1%} of the bandwidth roof")
            lines.append(f"n=2^{n_vars:<2} k={k} fused / level by level (medians) {r[FUSED][0] / r[LEVELS][0]:.3f}")
            for col in cols:
                col.free()
    return lines


def block_open(ctx, samples, max_log):
    n_vars = min(24, max_log)
    cols = [MLE.random(ctx, n_vars, 31 + j) for j in range(4)]
    tree = MerkleTree.commit(cols)
    tree.root()
    rng = random.Random(5)
    idx = [rng.randrange(1 << n_vars) for _ in range(64)]
    tree.open(idx, cols)
    times = []
    for _ in range(max(samples, 5)):
        t0 = time.perf_counter()
        tree.open(idx, cols)
        times.append((time.perf_counter() - t0) * 1e3)
    return [f"open of 64 rows, n=2^{n_vars} k=4 (upload of the indices, one gather launch, download of {64 * (n_vars + 4) * 32} bytes, one wait; wall clock): "
            f"median {statistics.median(times):.4f} ms  min {min(times):.4f} ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle.log"))
    a = ap.parse_args()
    lines = ["# tools/merkle_bench.py, BN254, MI355X; device ms between HIP events per build of the whole tree (average of 10 / 3 / 1 back-to-back "
             "builds at 2^16 / 2^20 / 2^24 rows after as many untimed ones); median and minimum of %d such samples" % a.samples,
             "# ZK_MERKLE_FUSE_LEVELS=%s (unset: the fused path uses the library's chosen tile); loadavg %s"
             % (os.environ.get("ZK_MERKLE_FUSE_LEVELS", "unset"), " ".join("%.2f" % v for v in os.getloadavg()))]
    ctx = zk_amd.Context(FIELD, 0)
    for block in (lambda: block_builds(ctx, a.samples, a.max_log), lambda: block_open(ctx, a.samples, a.max_log)):
        lines += block()
        print("\n".join(lines[-16:]), flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "a" if a.append else "w").write(text)


if __name__ == "__main__":
    main()
