"""Fractional-sum argument and lookup multiplicities on the device -> profiles/fsum.log (BN254, n = 16, 20, 24).

All paths of one size alternate in one process (zk_bench_fsum / zk_bench_gprod: device ms between HIP events, the average of `reps`
back-to-back runs after as many untimed ones); every row is median, minimum, maximum of the samples.

1. The fraction tree with p = ones: path 0, the switch's default (ZK_FSUM_TREE_FUSE levels per launch), against path 1, one level per
   launch; each against the bytes a tree must move -- 2^n elements of q read, 2 (2^n - 1) written -- at zk_bench_copy's rate, and against
   its multiplications -- one per node of the first level, three per node below -- at zk_bench_modmul's rate.  The default of the switch
   follows the faster path at n = 24 where the difference clears the run-to-run spread, else the fused path (fewer bytes).
2. The whole proof (path 2, p = ones) against zk_bench_gprod path 2 on the same table: the multiple found.
3. The multiplicities with the witness equal to the table (path 3, m = n) against the bytes of one pass over table and witness."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402

FIELD = zk_amd.BN254_FR
SWITCH = "ZK_FSUM_TREE_FUSE"


def stat(v):
    return statistics.median(v), min(v), max(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsum.log"))
    a = ap.parse_args()
    ctx = zk_amd.Context(FIELD, 0)
    copy = stat([ctx.bench_copy(1 << 30, 10) for _ in range(a.samples)])
    modmul = stat([ctx.bench_modmul(2000) for _ in range(a.samples)])
    lines = ["# tools/fsum_bench.py, BN254, MI355X; device ms between HIP events per run (average of `reps` back-to-back runs after as many "
             "untimed ones), %d such samples per path, the paths of one size alternating in one process; every row: median, minimum, maximum" % a.samples,
             "# %s=%s (unset: the default); loadavg %s" % (SWITCH, os.environ.get(SWITCH, "unset"), " ".join("%.2f" % v for v in os.getloadavg())),
             "zk_bench_copy 1 GiB: median %.0f GB/s  min %.0f  max %.0f | zk_bench_modmul: median %.3e modmul/s  min %.3e  max %.3e" % (copy + modmul)]
    print("\n".join(lines), flush=True)
    verdict = None
    paths = ("tree", "levels", "proof", "mult", "gprod")
    for n in (16, 20, 24):
        if n > a.max_log:
            continue
        got = []
        table = MLE.random(ctx, n, 90 + n)
        reps = {16: 50, 20: 20, 24: 5}[n]
        run = {"tree": lambda r: zk_amd.bench_fsum(table, 0, r), "levels": lambda r: zk_amd.bench_fsum(table, 1, r),
               "proof": lambda r: zk_amd.bench_fsum(table, 2, max(r // 5, 1)), "mult": lambda r: zk_amd.bench_fsum(table, 3, r),
               "gprod": lambda r: zk_amd.bench_gprod(table, 2, max(r // 5, 1))}
        for name in paths:   # warm: code objects, pool blocks
            run[name](1)
        ms = {name: [] for name in paths}
        for _ in range(a.samples):
            for name in paths:
                ms[name].append(run[name](reps))
        st = {name: stat(v) for name, v in ms.items()}
        moved, muls = 32 * ((1 << n) + 2 * ((1 << n) - 1)), (1 << (n - 1)) + 3 * ((1 << (n - 1)) - 1)
        floor_copy, floor_mul = moved / copy[0] / 1e6, muls / modmul[0] * 1e3
        for key, name in (("tree", "default route"), ("levels", "one level per launch")):
            med, lo, hi = st[key]
            got.append(f"n={n} tree (p = ones), {name}: median {med:.4f} ms  min {lo:.4f}  max {hi:.4f} (spread {(hi - lo) / med:.1%}) | the tree's own "
                       f"{moved / 2**20:.1f} MiB at the copy rate {floor_copy:.4f} ms ({floor_copy / med:.2f} of the time); {muls} multiplications at "
                       f"the modmul rate {floor_mul:.4f} ms ({floor_mul / med:.2f})")
        spread = max(st[k][2] - st[k][1] for k in ("tree", "levels"))
        got.append(f"n={n} one level per launch - default = {st['levels'][0] - st['tree'][0]:+.4f} ms (default / levels = "
                   f"{st['tree'][0] / st['levels'][0]:.3f}); the larger run-to-run spread (max - min) is {spread:.4f} ms")
        if n == 24:
            faster = "the default route" if st["tree"][0] < st["levels"][0] else "one level per launch"
            verdict = f"at n = 24 {faster} is faster" + (" by more than the spread" if abs(st["levels"][0] - st["tree"][0]) > spread else
                                                         ", within the spread: the fused path stays (fewer bytes)")
        (pm, pl, ph), (gm, gl, gh) = st["proof"], st["gprod"]
        got.append(f"n={n} whole proof (p = ones), device: median {pm:.3f} ms  min {pl:.3f}  max {ph:.3f} (spread {(ph - pl) / pm:.1%}) | zk_bench_gprod "
                   f"path 2 on the same table: median {gm:.3f} ms  min {gl:.3f}  max {gh:.3f} | fsum / gprod = {pm / gm:.2f}")
        mm, ml, mh = st["mult"]
        one_pass = 2 * (32 << n)
        got.append(f"n={n} multiplicities, witness = table (m = n): median {mm:.4f} ms  min {ml:.4f}  max {mh:.4f} (spread {(mh - ml) / mm:.1%}) | one pass "
                   f"over table and witness, {one_pass / 2**20:.1f} MiB, at the copy rate {one_pass / copy[0] / 1e6:.4f} ms ({one_pass / copy[0] / 1e6 / mm:.3f} of the time)")
        table.free()
        lines += got
        print("\n".join(got), flush=True)
    if verdict:
        lines.append("the default of %s that follows: %s" % (SWITCH, verdict))
        print(lines[-1], flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
