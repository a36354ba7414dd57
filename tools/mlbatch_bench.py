"""The batch multilinear commitment on the device, BN254, b = 1, Q = 32, n = 20 and 24.
1. zk_mlbatch_commit of k in {2, 4, 8} tables by wall clock beside k x zk_mlpcs_commit, and zk_mlbatch_open at m in {1, 2} points beside
   k m x zk_mlpcs_open (f = 0 and 4, as tools/mlpcs_bench.py), all in the same process: zk_mlpcs_* is the parent's code unchanged.  The
   condition: the batched opening is faster than the k m separate ones by more than the run-to-run spread at every (k, m) with k m >= 2.
2. The first fold of the codewords (zk_bench_mlbatch paths 1 and 2: device ms between HIP events): k_ml_combine_fold against the linear
   combination into a scratch layer followed by FRI's fold, alternating sample by sample, each also as a fraction of what zk_bench_copy
   reaches for the same bytes ((k + 1/2) 2^(n+b) 32 B fused, (k + 2 1/2) 2^(n+b) 32 B unfused).  What the default of
   ZK_MLBATCH_FUSE_FOLD follows.
3. One round (the fold joined to the sums) at POINTS_PER_PASS points in one pass (path 3) against as many single-point passes (path 4).
Output: profiles/mlbatch.log (--append adds a run to the log).

  python tools/mlbatch_bench.py [--samples 5] [--max-log 24] [--append] [--out profiles/mlbatch.log]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402

FIELD = zk_amd.BN254_FR
B, Q = 1, 32
POINTS_PER_PASS = 4   # mlbatch_kernels.cuh kMlPointsPerPass
COUNTS, POINTS, FINALS = (2, 4, 8), (1, 2), (0, 4)


def wall(fn, samples):
    fn()
    times = []
    for _ in range(samples):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def block_commit_open(ctx, samples, max_log):
    lines, failed = [], []
    shift = zk_amd.fe_from_int(FIELD, 5)
    seed = bytes(range(32))

    def sync(x):
        ctx.synchronize()
        return x

    for n in (20, 24):
        if n > max_log:
            continue
        tables = [MLE.random(ctx, n, 90 + n + 7 * j) for j in range(max(COUNTS))]
        pts = np.stack([zk_amd.fe_from_ints(FIELD, [0x5EED + 977 * i + 31 * j for i in range(n)]) for j in range(max(POINTS))])
        one, one_lo, one_hi = wall(lambda: sync(zk_amd.MultilinearCommitment.commit(tables[0], B, shift)).free(), samples)
        lines.append(f"n={n} b={B} zk_mlpcs_commit of one table: median {one:.3f} ms  min {one_lo:.3f}  max {one_hi:.3f}")
        single = zk_amd.MultilinearCommitment.commit(tables[0], B, shift)
        opened = {}
        for f in FINALS:
            opened[f] = wall(lambda: single.open(pts[0], f, Q, seed), samples)
            lines.append(f"n={n} b={B} f={f} Q={Q} zk_mlpcs_open of one table at one point: median {opened[f][0]:.3f} ms  min {opened[f][1]:.3f}  max {opened[f][2]:.3f} "
                         f"({zk_amd.mlpcs_proof_bytes(n, B, f, Q)} proof bytes)")
        single.free()
        for k in COUNTS:
            med, lo, hi = wall(lambda: sync(zk_amd.MultilinearBatchCommitment.commit(tables[:k], B, shift)).free(), samples)
            lines.append(f"n={n} b={B} k={k} zk_mlbatch_commit: median {med:.3f} ms  min {lo:.3f}  max {hi:.3f} | {k} x zk_mlpcs_commit = {k * one:.3f} ms | "
                         f"ratio {med / (k * one):.3f}")
            com = zk_amd.MultilinearBatchCommitment.commit(tables[:k], B, shift)
            for m in POINTS:
                for f in FINALS:
                    med, lo, hi = wall(lambda: com.open(pts[:m], f, Q, seed), samples)
                    sep = k * m * opened[f][0]
                    spread = (hi - lo) + k * m * (opened[f][2] - opened[f][1])
                    ok = sep - med > spread
                    if not ok:
                        failed.append((n, k, m, f))
                    lines.append(f"n={n} b={B} f={f} Q={Q} k={k} m={m} zk_mlbatch_open: median {med:.3f} ms  min {lo:.3f}  max {hi:.3f} "
                                 f"({zk_amd.mlbatch_proof_bytes(n, k, m, B, f, Q)} proof bytes against {k * m} x {zk_amd.mlpcs_proof_bytes(n, B, f, Q)}) | "
                                 f"{k * m} x zk_mlpcs_open = {sep:.3f} ms | ratio {med / sep:.3f} = {sep / med:.2f} x faster | spread of both sides "
                                 f"{spread:.3f} ms: {'faster by more than the spread' if ok else 'NOT faster by more than the spread'}")
            com.free()
        for t in tables:
            t.free()
    lines.append("the condition (every measured (k, m) with k m >= 2 faster than the k m separate openings by more than the spread): "
                 + ("holds" if not failed else "FAILS at (n, k, m, f) = %s" % failed))
    return lines


def block_device(ctx, samples, max_log):
    lines, verdicts = [], []
    shift = zk_amd.fe_from_int(FIELD, 5)
    for n in (20, 24):
        if n > max_log:
            continue
        reps = 10 if n <= 20 else 3
        tables = [MLE.random(ctx, n, 50 + n + 3 * j) for j in range(max(COUNTS))]
        for k in COUNTS:
            com = zk_amd.MultilinearBatchCommitment.commit(tables[:k], B, shift)
            for path in (1, 2):   # warm: code objects, pool blocks
                zk_amd.bench_mlbatch(com, 1, path, 1)
            got = {1: [], 2: []}
            for _ in range(samples):   # alternating, so that a drift of the machine hits both
                for path in (1, 2):
                    got[path].append(zk_amd.bench_mlbatch(com, 1, path, reps))
            stat = {p: (statistics.median(v), min(v), max(v)) for p, v in got.items()}
            layer = 32 << (n + B)
            moved = {1: (k + 0.5) * layer, 2: (k + 2.5) * layer}
            for p, name in ((1, "fused  "), (2, "unfused")):
                med, lo, hi = stat[p]
                copy_ms = moved[p] / (ctx.bench_copy(int(moved[p]) // 2 & ~15, 5) * 1e6)   # a plain copy of half as many bytes reads and writes as many
                lines.append(f"n={n} k={k} first fold {name}: median {med:.4f} ms  min {lo:.4f}  max {hi:.4f} (spread {(hi - lo) / med:.1%}) | moves "
                             f"{moved[p] / 2**20:.0f} MiB: {moved[p] / med / 1e6:.0f} GB/s; zk_bench_copy moves them in {copy_ms:.4f} ms: the kernel runs at "
                             f"{copy_ms / med:.3f} of the copy's rate")
            spread = max(stat[p][2] - stat[p][1] for p in (1, 2))
            diff = stat[2][0] - stat[1][0]
            verdicts.append((n, k, diff, spread))
            lines.append(f"n={n} k={k} unfused - fused = {diff:+.4f} ms (fused / unfused = {stat[1][0] / stat[2][0]:.3f}); the larger run-to-run spread (max - min) is "
                         f"{spread:.4f} ms")
            if k == COUNTS[0]:   # the rounds read the first table only
                for path in (3, 4):
                    zk_amd.bench_mlbatch(com, 1, path, 1)
                rounds = {3: [], 4: []}
                for _ in range(samples):
                    for path in (3, 4):
                        rounds[path].append(zk_amd.bench_mlbatch(com, 1, path, reps))
                rs = {p: (statistics.median(v), min(v), max(v)) for p, v in rounds.items()}
                alg = (32 << n) + (32 << (n - 1))   # T read once, the folded half written once
                for p, name in ((3, f"one pass at {POINTS_PER_PASS} points "), (4, f"{POINTS_PER_PASS} single-point passes")):
                    med, lo, hi = rs[p]
                    lines.append(f"n={n} one round (2^{n} -> 2^{n - 1}, fold joined to the sums), {name}: median {med:.4f} ms  min {lo:.4f}  max {hi:.4f} "
                                 f"(spread {(hi - lo) / med:.1%}); one pass moves {alg / 2**20:.0f} MiB: {alg / rs[3][0] / 1e6:.0f} GB/s in the multi-point kernel")
                rspread = max(rs[p][2] - rs[p][1] for p in (3, 4))
                rdiff = rs[4][0] - rs[3][0]
                lines.append(f"n={n} single-point passes - one pass = {rdiff:+.4f} ms (one pass / single passes = {rs[3][0] / rs[4][0]:.3f}); the larger spread is "
                             f"{rspread:.4f} ms: the multi-point kernel is {'faster by more than the spread' if rdiff > rspread else 'NOT faster by more than the spread'}")
            com.free()
        for t in tables:
            t.free()
    at = [v for v in verdicts if v[0] == max(x[0] for x in verdicts)] if verdicts else []
    if at:
        fused_wins = all(d > s for _, _, d, s in at)
        unfused_wins = all(-d > s for _, _, d, s in at)
        lines.append("the default of ZK_MLBATCH_FUSE_FOLD that follows at n = %d: %s" % (
            at[0][0], "fused (1)" if fused_wins else "unfused (0)" if unfused_wins else "no route clears the spread at every k: fused (1) stays, it moves fewer bytes"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlbatch.log"))
    a = ap.parse_args()
    lines = ["# tools/mlbatch_bench.py, BN254, MI355X, b = %d, Q = %d; commit / open: wall clock of the whole call (each ends in a host wait), median, minimum "
             "and maximum of %d calls after one untimed; first fold and rounds: device ms between HIP events (average of 10 / 3 back-to-back runs at "
             "n = 20 / 24 after as many untimed ones), %d such samples per path, the paths alternating" % (B, Q, a.samples, a.samples),
             "# ZK_MLBATCH_FUSE_FOLD=%s (unset: the default route); loadavg %s" % (os.environ.get("ZK_MLBATCH_FUSE_FOLD", "unset"),
                                                                                   " ".join("%.2f" % v for v in os.getloadavg()))]
    ctx = zk_amd.Context(FIELD, 0)
    for block in (lambda: block_device(ctx, a.samples, a.max_log), lambda: block_commit_open(ctx, a.samples, a.max_log)):
        got = block()
        lines += got
        print("\n".join(got), flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "a" if a.append else "w").write(text)


if __name__ == "__main__":
    main()
