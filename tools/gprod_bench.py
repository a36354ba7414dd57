"""Grand-product argument on the device -> profiles/gprod.log (BN254, n = 16, 20, 24).

1. The product tree (zk_bench_gprod: device ms between HIP events): path 0, the switch's default (ZK_GPROD_TREE_FUSE levels per launch),
   against path 1, one level per launch, alternating; each against the bytes a tree must move -- 2^n elements read, 2^n - 1 written --
   at zk_bench_copy's rate and against its 2^n - 1 multiplications at zk_bench_modmul's rate.  The default of the switch follows the
   faster path at n = 24 where the difference clears the run-to-run spread, else the fused path (fewer bytes).
2. The whole proof (path 2: device ms, everything zk_gprod_prove enqueues) and zk_gprod_prove itself (wall clock of the call, with its one
   host wait) against what a user could assemble before this call existed, on the same table: the halves of every level by
   partial_evaluate(0, [0]) / (0, [1]) and their product by prod_reduce, then per layer zk_eq_table and zk_sumcheck_prove_terms on
   (E, A, B) with its host wait and the point's way back to the device; and against zk_bench_prove_partial (k = 3, D = 3) at n - 1
   variables, the top layer's sumcheck alone."""
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
from zk_amd import ProductPoly, gkr  # noqa: E402

FIELD = zk_amd.BN254_FR


def stat(v):
    return statistics.median(v), min(v), max(v)


def composition(ctx, table, n):
    """the argument's work by the calls that existed before it (no transcript chaining: each sumcheck starts its own); returns the product"""
    zero, one = zk_amd.fe_from_int(FIELD, 0), zk_amd.fe_from_int(FIELD, 1)
    levels = [table]
    for j in range(n - 1, -1, -1):
        lo, hi = levels[0].partial_evaluate(0, zero), levels[0].partial_evaluate(0, one)
        levels.insert(0, ProductPoly([lo, hi]).prod_reduce_device())
        lo.free()
        hi.free()
    product = levels[0].evaluation_slice()[0]
    point = zk_amd.fe_from_ints(FIELD, [5])   # a stand-in for r_1 = (tau_0)
    claim = product
    for j in range(1, n):
        up = levels[j + 1]
        e, a, b = gkr.eq_table(ctx, point), up.partial_evaluate(0, zero), up.partial_evaluate(0, one)
        rp, ch, fin = gkr.prove_partial_terms(gkr.SumOfProductsPoly([[e, a, b]]), 3, claim, consume=True)
        for x in (e, a, b):
            x.free()
        point = np.concatenate([ch[:1], ch])   # a stand-in for (tau, rho): j + 1 elements
        claim = fin[1]
    for lv in levels[:-1]:
        lv.free()
    return product


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gprod.log"))
    a = ap.parse_args()
    ctx = zk_amd.Context(FIELD, 0)
    copy = stat([ctx.bench_copy(1 << 30, 10) for _ in range(a.samples)])
    modmul = stat([ctx.bench_modmul(2000) for _ in range(a.samples)])
    lines = ["# tools/gprod_bench.py, BN254, MI355X; tree and proof (device): ms between HIP events per run (average of `reps` back-to-back runs after "
             "as many untimed ones), %d such samples per path, the paths alternating; zk_gprod_prove and the composition: wall clock of the whole "
             "call, %d calls after one untimed; every row: median, minimum, maximum" % (a.samples, a.samples),
             "# ZK_GPROD_TREE_FUSE=%s (unset: the default); loadavg %s" % (os.environ.get("ZK_GPROD_TREE_FUSE", "unset"), " ".join("%.2f" % v for v in os.getloadavg())),
             "zk_bench_copy 1 GiB: median %.0f GB/s  min %.0f  max %.0f | zk_bench_modmul: median %.3e modmul/s  min %.3e  max %.3e" % (copy + modmul)]
    print("\n".join(lines), flush=True)
    verdict = None
    for n in (16, 20, 24):
        if n > a.max_log:
            continue
        got = []
        table = MLE.random(ctx, n, 70 + n)
        reps = {16: 50, 20: 20, 24: 5}[n]
        for path in (0, 1, 2):   # warm: code objects, pool blocks
            zk_amd.bench_gprod(table, path, 1)
        ms = {0: [], 1: [], 2: []}
        for _ in range(a.samples):
            for path in (0, 1, 2):
                ms[path].append(zk_amd.bench_gprod(table, path, reps if path < 2 else max(reps // 5, 1)))
        moved, muls = 32 * ((2 << n) - 1), (1 << n) - 1
        floor_copy, floor_mul = moved / copy[0] / 1e6, muls / modmul[0] * 1e3
        st = {p: stat(v) for p, v in ms.items()}
        for p, name in ((0, "default route"), (1, "one level per launch")):
            med, lo, hi = st[p]
            got.append(f"n={n} tree, {name}: median {med:.4f} ms  min {lo:.4f}  max {hi:.4f} (spread {(hi - lo) / med:.1%}) | the tree's own "
                       f"{moved / 2**20:.1f} MiB at the copy rate {floor_copy:.4f} ms ({floor_copy / med:.2f} of the time); {muls} multiplications at "
                       f"the modmul rate {floor_mul:.4f} ms ({floor_mul / med:.2f})")
        spread = max(st[p][2] - st[p][1] for p in (0, 1))
        got.append(f"n={n} one level per launch - default = {st[1][0] - st[0][0]:+.4f} ms (default / levels = {st[0][0] / st[1][0]:.3f}); the larger "
                   f"run-to-run spread (max - min) is {spread:.4f} ms")
        if n == 24:
            faster = "the default route" if st[0][0] < st[1][0] else "one level per launch"
            verdict = f"at n = 24 {faster} is faster" + (" by more than the spread" if abs(st[1][0] - st[0][0]) > spread else
                                                         ", within the spread: the fused path stays (fewer bytes)")
        med, lo, hi = st[2]
        got.append(f"n={n} whole proof, device: median {med:.3f} ms  min {lo:.3f}  max {hi:.3f} (spread {(hi - lo) / med:.1%})")
        seed = bytes(range(32))
        zk_amd.grand_product_prove(table, seed)
        wall = []
        for _ in range(a.samples):
            t0 = time.perf_counter()
            zk_amd.grand_product_prove(table, seed)
            wall.append((time.perf_counter() - t0) * 1e3)
        pw = stat(wall)
        composition(ctx, table, n)
        comp = []
        for _ in range(a.samples):
            t0 = time.perf_counter()
            composition(ctx, table, n)
            comp.append((time.perf_counter() - t0) * 1e3)
        cw = stat(comp)
        got.append(f"n={n} zk_gprod_prove, wall clock: median {pw[0]:.3f} ms  min {pw[1]:.3f}  max {pw[2]:.3f} | the composition of public calls on "
                   f"the same table: median {cw[0]:.3f} ms  min {cw[1]:.3f}  max {cw[2]:.3f} | proof / composition = {pw[0] / cw[0]:.3f}")
        tabs = [MLE.random(ctx, n - 1, 200 + i) for i in range(3)]
        zero = zk_amd.fe_from_int(FIELD, 0)
        top = stat(zk_amd.bench_prove_partial(ProductPoly(tabs), 3, zero, reps=a.samples + 1)[1:])
        for x in tabs:
            x.free()
        got.append(f"n={n} zk_bench_prove_partial k = 3, D = 3 at {n - 1} variables (the top layer alone): median {top[0]:.3f} ms  min {top[1]:.3f}  "
                   f"max {top[2]:.3f} | proof / top layer = {pw[0] / top[0]:.3f}")
        table.free()
        lines += got
        print("\n".join(got), flush=True)
    if verdict:
        lines.append("the default of ZK_GPROD_TREE_FUSE that follows: " + verdict)
        print(lines[-1], flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
