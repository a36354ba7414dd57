"""The multilinear polynomial commitment on the device, BN254, Q = 32.
1. zk_mlpcs_commit and zk_mlpcs_open by wall clock (each ends in a host wait) at n = 20 and 24, b = 1 and 2, f = 0 and 4, beside
   zk_fri_prove at d = n, a = 1 with the same b, f, Q in the same process (its code is the parent's) and zk_fri_lde, which zk_fri_prove
   runs first and the opening does not (the commitment did): the opening does that proof's work plus the sumcheck side.
2. The sumcheck side alone (zk_bench_mlpcs_round: device ms between HIP events over all n rounds, no host wait): the fused round kernel
   against the eq-table route, the two alternating sample by sample, with the spread of each; and the bytes each route moves, counted
   from the shapes, against the algorithmic bytes (round 0: T_0 read once; round r >= 1: T_{r-1} read once, T_r written once).
3. Which route is faster at n = 24 by more than the spread: what the default of ZK_MLPCS_ROUND follows.
Output: profiles/mlpcs.log (--append adds a run to the log).

  python tools/mlpcs_bench.py [--samples 7] [--max-log 24] [--append] [--out profiles/mlpcs.log]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402
from zk_amd import UnivariatePolynomial as Poly  # noqa: E402

FIELD = zk_amd.BN254_FR
Q = 32
LO_BITS, RUN_MIN_BITS, RUNS_TARGET_LOG, MAX_BLOCKS = 9, 6, 11, 2048   # mlpcs_kernels.cuh kMlLoBits, kMlRunMinBits, kMlRunsTargetLog; host_core.hpp kMaxGrid


def wall(fn, samples):
    fn()
    times = []
    for _ in range(samples):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def algorithmic_bytes(n):
    """per round: T_0 read once in round 0; T_{r-1} read once and T_r written once in round r >= 1"""
    return [32 << n] + [(32 << (n - r + 1)) + (32 << (n - r)) for r in range(1, n)]


def fused_bytes(n):
    """what the fused route moves: the algorithmic bytes, the Lo table once per workgroup and one Hi entry per run (both from L2 after the
    first touch), and the suffix tables' build (written once)"""
    out = []
    for r, alg in enumerate(algorithmic_bytes(n)):
        m = n - r - 1
        L = min(m, LO_BITS)
        runs = 1 << (m - min(L, max(RUN_MIN_BITS, m - RUNS_TARGET_LOG)))
        blocks = 1 if m < RUN_MIN_BITS else min(-(-runs // 4), MAX_BLOCKS)
        out.append(alg + blocks * (32 << L) + 32 * runs)
    return out


def tables_bytes(n):
    """what the eq-table route moves: E_0 written once (2^n elements); per round both tables read by the round sums; per round r >= 1
    two folds before them, each reading 2^(n-r+1) and writing 2^(n-r) elements"""
    out = []
    for r in range(n):
        sums = 2 * (32 << (n - r))
        folds = 2 * ((32 << (n - r + 1)) + (32 << (n - r))) if r else 32 << n
        out.append(sums + folds)
    return out


def block_open(ctx, samples, max_log):
    lines = []
    shift = zk_amd.fe_from_int(FIELD, 5)
    seed = bytes(range(32))

    def sync(x):
        ctx.synchronize()
        return x

    for n in (20, 24):
        if n > max_log:
            continue
        table = MLE.random(ctx, n, 90 + n)
        poly = Poly.new(ctx, table.evaluation_slice())   # the same 2^n numbers as coefficients, for zk_fri_prove
        point = zk_amd.fe_from_ints(FIELD, [0x5EED + 977 * j for j in range(n)])
        for b in (1, 2):
            med, lo, hi = wall(lambda: sync(zk_amd.MultilinearCommitment.commit(table, b, shift)).free(), samples)
            lines.append(f"n={n} b={b} zk_mlpcs_commit (interpolate, the LDE to 2^{n + b} points, the tree over 2^{n + b - 1} rows of two columns; waited "
                         f"for): median {med:.3f} ms  min {lo:.3f}  max {hi:.3f}")
            lde, lde_lo, _ = wall(lambda: sync(zk_amd.fri_lde(poly, n + b, shift)).free(), samples)
            com = zk_amd.MultilinearCommitment.commit(table, b, shift)
            for f in (0, 4):
                fri, fri_lo, fri_hi = wall(lambda: zk_amd.fri_prove(poly, n, b, 1, f, Q, shift, seed), samples)
                opn, opn_lo, opn_hi = wall(lambda: com.open(point, f, Q, seed), samples)
                base = fri - lde
                lines.append(f"n={n} b={b} f={f} Q={Q} zk_mlpcs_open median {opn:.3f} ms  min {opn_lo:.3f}  max {opn_hi:.3f} ({zk_amd.mlpcs_proof_bytes(n, b, f, Q)} proof "
                             f"bytes) | zk_fri_prove d={n} a=1 median {fri:.3f} ms  min {fri_lo:.3f}  max {fri_hi:.3f}, of which its LDE (zk_fri_lde, waited for) "
                             f"{lde:.3f} ms: the FRI work alone {base:.3f} ms | opening - FRI work = {opn - base:+.3f} ms, ratio {opn / base:.3f}")
            com.free()
        poly.free()
        table.free()
    return lines


def block_rounds(ctx, samples, max_log):
    lines, verdict = [], None
    for n in (20, 24):
        if n > max_log:
            continue
        table = MLE.random(ctx, n, 50 + n)
        reps = 10 if n <= 20 else 3
        for path in (1, 2):   # warm: code objects, pool blocks
            zk_amd.bench_mlpcs_round(table, path, 1)
        got = {1: [], 2: []}
        for _ in range(samples):   # alternating, so that a drift of the machine hits both
            for path in (1, 2):
                got[path].append(zk_amd.bench_mlpcs_round(table, path, reps))
        table.free()
        alg, fb, tb = sum(algorithmic_bytes(n)), sum(fused_bytes(n)), sum(tables_bytes(n))
        stat = {p: (statistics.median(v), min(v), max(v)) for p, v in got.items()}
        for p, name, moved in ((1, "fused ", fb), (2, "tables", tb)):
            med, lo, hi = stat[p]
            lines.append(f"n={n} sumcheck side, all {n} rounds, {name}: median {med:.4f} ms  min {lo:.4f}  max {hi:.4f} (spread {(hi - lo) / med:.1%}) | moves "
                         f"{moved / 2**20:.1f} MiB = {moved / alg:.3f} x the algorithmic {alg / 2**20:.1f} MiB: {moved / med / 1e6:.0f} GB/s moved, "
                         f"{alg / med / 1e6:.0f} GB/s algorithmic")
        spread = max((stat[p][2] - stat[p][1]) for p in (1, 2))
        diff = stat[2][0] - stat[1][0]
        lines.append(f"n={n} tables - fused = {diff:+.4f} ms (fused / tables = {stat[1][0] / stat[2][0]:.3f}); the larger run-to-run spread (max - min) is {spread:.4f} ms")
        for r in (0, 1, 2, 3):
            lines.append(f"n={n} round {r}: algorithmic {algorithmic_bytes(n)[r] / 2**20:8.2f} MiB | fused moves {fused_bytes(n)[r] / 2**20:8.2f} MiB | tables moves "
                         f"{tables_bytes(n)[r] / 2**20:8.2f} MiB (counted from the shapes)")
        if n == 24:
            verdict = "fused (ZK_MLPCS_ROUND=1)" if diff > spread else "tables (ZK_MLPCS_ROUND=0): the fused kernel does not clear the spread"
    if verdict:
        lines.append(f"the default of ZK_MLPCS_ROUND that follows at n = 24: {verdict}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlpcs.log"))
    a = ap.parse_args()
    lines = ["# tools/mlpcs_bench.py, BN254, MI355X, Q = %d; commit / open / zk_fri_prove: wall clock of the whole call (each ends in a host wait), median, "
             "minimum and maximum of %d calls after one untimed; sumcheck side: device ms between HIP events per opening (average of 10 / 3 "
             "back-to-back ones at n = 20 / 24 after as many untimed ones), %d such samples per route, the routes alternating" % (Q, a.samples, a.samples),
             "# ZK_MLPCS_ROUND=%s (unset: the default route); loadavg %s" % (os.environ.get("ZK_MLPCS_ROUND", "unset"), " ".join("%.2f" % v for v in os.getloadavg()))]
    ctx = zk_amd.Context(FIELD, 0)
    for block in (lambda: block_rounds(ctx, a.samples, a.max_log), lambda: block_open(ctx, a.samples, a.max_log)):
        got = block()
        lines += got
        print("\n".join(got), flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "a" if a.append else "w").write(text)


if __name__ == "__main__":
    main()
