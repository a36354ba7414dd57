"""Zerocheck argument on the device -> profiles/zerocheck.log (BN254, n = 20 and 24; zk_bench_zerocheck: device ms between HIP events).

1. The price of the gate interpreter: the gate x0 (k = 1, d = 1) does the work of the multilinear commitment's round kernel, so its
   round-0 launch (path 1), its round-1 launch (path 2: fold joined to the sums) and its whole proof (path 0: every round, with the
   transcript steps) stand beside zk_bench_mlpcs_round's fused path (k_ml_round, every round, no transcript) on the same table in the
   same run, alternating.
2. The Plonk gate (k = 8, T = 5, d = 3): round 0, round 1 and the whole proof beside the time their algorithmic bytes -- k columns read,
   and from round 1 on k half-columns written -- would take at zk_bench_copy's rate in the same run, and beside the multiplications a
   row costs at zk_bench_modmul's rate: which bound binds.
Every row: median, minimum, maximum over --samples repetitions."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402

FIELD = zk_amd.BN254_FR
X0 = (1, [(1, (0,))])
PLONK = (8, [(1, (3, 0)), (1, (4, 1)), (1, (5, 0, 1)), (1, (6, 2)), (1, (7,))])   # a, b, c, qL, qR, qM, qO, qC
# multiplications per x' of a Plonk round: (d + 1) = 4 points x (5 products in the gate + the weight), and 2 per column for the fold
PLONK_MULS_SUMS, PLONK_MULS_FOLD = 4 * (5 + 1), 2 * 8


def stat(v):
    return statistics.median(v), min(v), max(v)


def row(name, v):
    med, lo, hi = stat(v)
    return f"{name}: median {med:.4f} ms  min {lo:.4f}  max {hi:.4f} (spread {(hi - lo) / med:.1%})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zerocheck.log"))
    a = ap.parse_args()
    ctx = zk_amd.Context(FIELD, 0)
    copy = stat([ctx.bench_copy(1 << 30, 10) for _ in range(a.samples)])
    modmul = stat([ctx.bench_modmul(2000) for _ in range(a.samples)])
    lines = ["# tools/zerocheck_bench.py, BN254, MI355X; device ms between HIP events per run (average of `reps` back-to-back runs after as many "
             "untimed ones), %d such samples per row, the rows of a block alternating; every row: median, minimum, maximum" % a.samples,
             "# loadavg %s" % " ".join("%.2f" % v for v in os.getloadavg()),
             "zk_bench_copy 1 GiB: median %.0f GB/s  min %.0f  max %.0f | zk_bench_modmul: median %.3e modmul/s  min %.3e  max %.3e" % (copy + modmul)]
    print("\n".join(lines), flush=True)
    gx0, gpl = zk_amd.Gate(FIELD, *X0), zk_amd.Gate(FIELD, *PLONK)
    for n in (20, 24):
        if n > a.max_log:
            continue
        reps = {20: 20, 24: 3}[n]
        tabs = [MLE.random(ctx, n, 90 + i) for i in range(8)]
        runs = {"x0 round 0": lambda: zk_amd.bench_zerocheck(tabs[:1], gx0, 1, reps), "x0 round 1": lambda: zk_amd.bench_zerocheck(tabs[:1], gx0, 2, reps),
                "x0 whole proof": lambda: zk_amd.bench_zerocheck(tabs[:1], gx0, 0, max(reps // 3, 1)),
                "k_ml_round, every round (zk_bench_mlpcs_round path 1)": lambda: zk_amd.bench_mlpcs_round(tabs[0], 1, max(reps // 3, 1)),
                "plonk round 0": lambda: zk_amd.bench_zerocheck(tabs, gpl, 1, reps), "plonk round 1": lambda: zk_amd.bench_zerocheck(tabs, gpl, 2, reps),
                "plonk whole proof": lambda: zk_amd.bench_zerocheck(tabs, gpl, 0, max(reps // 3, 1))}
        ms = {name: [] for name in runs}
        for fn in runs.values():   # warm: code objects, pool blocks
            fn()
        for _ in range(a.samples):
            for name, fn in runs.items():
                ms[name].append(fn())
        got = [row(f"n={n} {name}", v) for name, v in ms.items()]
        med = {name: statistics.median(v) for name, v in ms.items()}
        spread = max(max(v) - min(v) for name, v in ms.items() if name.startswith("x0 whole") or name.startswith("k_ml_round"))
        gap = med["x0 whole proof"] - med["k_ml_round, every round (zk_bench_mlpcs_round path 1)"]
        got.append(f"n={n} x0 whole proof - k_ml_round's rounds = {gap:+.4f} ms (ratio {med['x0 whole proof'] / med['k_ml_round, every round (zk_bench_mlpcs_round path 1)']:.3f}); "
                   f"the larger run-to-run spread (max - min) of the two is {spread:.4f} ms: the interpreter (and the {n} transcript steps the proof "
                   f"has and the other has not) costs {'more than' if gap > spread else 'no more than'} the spread")
        # x0's own rounds against their bytes
        for name, moved in (("x0 round 0", 32 << n), ("x0 round 1", (32 << n) + (32 << (n - 1)))):
            floor = moved / copy[0] / 1e6
            got.append(f"n={n} {name}: {moved / 2**20:.0f} MiB at the copy rate {floor:.4f} ms ({floor / med[name]:.2f} of the time)")
        half = 1 << (n - 1)
        for name, moved, muls in (("plonk round 0", 8 * (32 << n), half * PLONK_MULS_SUMS),
                                  ("plonk round 1", 8 * ((32 << n) + (32 << (n - 1))), (half // 2) * (PLONK_MULS_SUMS + PLONK_MULS_FOLD)),
                                  ("plonk whole proof", 8 * ((32 << n) + 2 * (32 << n) + (32 << n)), 2 * half * PLONK_MULS_SUMS + half * PLONK_MULS_FOLD)):
            floor_copy, floor_mul = moved / copy[0] / 1e6, muls / modmul[0] * 1e3
            binds = "the multiplier" if floor_mul > floor_copy else "memory"
            got.append(f"n={n} {name}: its algorithmic {moved / 2**20:.0f} MiB at the copy rate {floor_copy:.4f} ms ({floor_copy / med[name]:.2f} of the "
                       f"time); its {muls} multiplications at the modmul rate {floor_mul:.4f} ms ({floor_mul / med[name]:.2f}): {binds} binds")
        for t in tabs:
            t.free()
        lines += got
        print("\n".join(got), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
