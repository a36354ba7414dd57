"""Wiring permutation argument on the device -> profiles/perm.log (BN254, (n, k) = (20, 3), (20, 8), (21, 4)).

1. The fingerprint table F and its whole product tree (zk_bench_perm: device ms between HIP events): path 3, the fused route (one
   launch of k_perm_tree<A> writes F and the tree's first A levels, then the tree's own launches), against path 1, the unfused route
   (k_perm_leaves, then zk_mle_product_tree's launches over F), alternating; each against the bytes the route must move at
   zk_bench_copy's rate.  Child processes repeat both paths under ZK_GPROD_TREE_FUSE = 1, 2, 3: each A of the fused kernel (A = min(the
   switch, 2)) against the tree that the unfused route runs with that many levels per launch.  The default of ZK_PERM_FUSE follows the
   faster route where the difference clears the run-to-run spread.
2. The whole proof (path 2: device ms, everything zk_perm_prove enqueues and the 2 k evaluations) against zk_bench_gprod's whole proof on
   the materialised F of the same N, and zk_perm_prove itself (wall clock of the call, with its two host waits)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402

FIELD = zk_amd.BN254_FR
SHAPES = ((20, 3), (20, 8), (21, 4))
PERM_MAX_FUSE = 2   # kPermMaxFuse


def stat(v):
    return statistics.median(v), min(v), max(v)


def kappa(k):
    return (k - 1).bit_length()


def routes(ctx, n, k, samples, reps):
    """{path: [ms]} for the two tree routes, alternating"""
    w = [MLE.random(ctx, n, 10 + i) for i in range(k)]
    sg = [MLE.random(ctx, n, 40 + i) for i in range(k)]
    for path in (3, 1):   # warm: code objects, pool blocks
        zk_amd.bench_perm(w, sg, path, 1)
    ms = {3: [], 1: []}
    for _ in range(samples):
        for path in (3, 1):
            ms[path].append(zk_amd.bench_perm(w, sg, path, reps))
    return w, sg, ms


def child(a):
    ctx = zk_amd.Context(FIELD, 0)
    fuse = os.environ.get("ZK_GPROD_TREE_FUSE", "unset")
    for n, k in SHAPES:
        if n > a.max_log:
            continue
        w, sg, ms = routes(ctx, n, k, a.samples, a.reps)
        f, u = stat(ms[3]), stat(ms[1])
        print(f"n={n} k={k} ZK_GPROD_TREE_FUSE={fuse}: fused route (A = {min(int(fuse), PERM_MAX_FUSE)}) median {f[0]:.4f} ms  min {f[1]:.4f}  max {f[2]:.4f} | "
              f"unfused route median {u[0]:.4f} ms  min {u[1]:.4f}  max {u[2]:.4f} | unfused - fused = {u[0] - f[0]:+.4f} ms", flush=True)
        for t in w + sg:
            t.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=21)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perm.log"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    ctx = zk_amd.Context(FIELD, 0)
    copy = stat([ctx.bench_copy(1 << 30, 10) for _ in range(a.samples)])
    lines = ["# tools/perm_bench.py, BN254, MI355X; routes and proofs (device): ms between HIP events per run (average of `reps` back-to-back runs "
             "after as many untimed ones), %d such samples per path, the paths alternating; zk_perm_prove: wall clock of the whole call, %d calls "
             "after one untimed; every row: median, minimum, maximum" % (a.samples, a.samples),
             "# ZK_PERM_FUSE=%s ZK_GPROD_TREE_FUSE=%s (unset: the defaults); loadavg %s" % (os.environ.get("ZK_PERM_FUSE", "unset"),
                                                                                          os.environ.get("ZK_GPROD_TREE_FUSE", "unset"),
                                                                                          " ".join("%.2f" % v for v in os.getloadavg())),
             "zk_bench_copy 1 GiB: median %.0f GB/s  min %.0f  max %.0f" % copy]
    print("\n".join(lines), flush=True)
    verdicts = []
    for n, k in SHAPES:
        if n > a.max_log:
            continue
        N, got = n + kappa(k) + 1, []
        w, sg, ms = routes(ctx, n, k, a.samples, a.reps)
        st = {p: stat(v) for p, v in ms.items()}
        cols, F = 64 * k * (1 << n), 32 << N
        moved = {3: cols + 2 * F + (F >> PERM_MAX_FUSE), 1: cols + 3 * F}   # columns in, F out, (F in again,) the heap out, the tree's next level in
        for p, name in ((3, "fused route (k_perm_tree<%d>, then the tree)" % PERM_MAX_FUSE), (1, "unfused route (k_perm_leaves, then the tree over F)")):
            med, lo, hi = st[p]
            floor = moved[p] / copy[0] / 1e6
            got.append(f"n={n} k={k} N={N} F and its tree, {name}: median {med:.4f} ms  min {lo:.4f}  max {hi:.4f} (spread {(hi - lo) / med:.1%}) | "
                       f"its {moved[p] / 2**20:.0f} MiB at the copy rate {floor:.4f} ms ({floor / med:.2f} of the time)")
        spread = max(st[p][2] - st[p][1] for p in (3, 1))
        diff = st[1][0] - st[3][0]
        got.append(f"n={n} k={k} unfused - fused = {diff:+.4f} ms (fused / unfused = {st[3][0] / st[1][0]:.3f}); the larger run-to-run spread "
                   f"(max - min) is {spread:.4f} ms")
        verdicts.append((n, k, diff, spread))
        # the whole proof against the grand product of a materialised F of the same N
        fp = zk_amd.perm_fingerprint(w, sg, zk_amd.fe_from_int(FIELD, 2), zk_amd.fe_from_int(FIELD, 1))
        for _ in range(2):
            zk_amd.bench_perm(w, sg, 2, 1)
            zk_amd.bench_gprod(fp, 2, 1)
        pm, gp = [], []
        for _ in range(a.samples):
            pm.append(zk_amd.bench_perm(w, sg, 2, 1))
            gp.append(zk_amd.bench_gprod(fp, 2, 1))
        fp.free()
        pm, gp = stat(pm), stat(gp)
        got.append(f"n={n} k={k} whole proof on the default route, device: median {pm[0]:.3f} ms  min {pm[1]:.3f}  max {pm[2]:.3f} | zk_gprod_prove's device work on a "
                   f"materialised F (N = {N}): median {gp[0]:.3f} ms  min {gp[1]:.3f}  max {gp[2]:.3f} | perm - gprod = {pm[0] - gp[0]:+.3f} ms "
                   f"(the launch that writes F and the {2 * k} evaluations)")
        seed, beta, gamma = bytes(range(32)), zk_amd.fe_from_int(FIELD, 12345), zk_amd.fe_from_int(FIELD, 67890)
        zk_amd.permutation_prove(w, sg, beta, gamma, seed)
        wall = []
        for _ in range(a.samples):
            t0 = time.perf_counter()
            zk_amd.permutation_prove(w, sg, beta, gamma, seed)
            wall.append((time.perf_counter() - t0) * 1e3)
        pw = stat(wall)
        got.append(f"n={n} k={k} zk_perm_prove, wall clock (two host waits): median {pw[0]:.3f} ms  min {pw[1]:.3f}  max {pw[2]:.3f}")
        for t in w + sg:
            t.free()
        lines += got
        print("\n".join(got), flush=True)
    ctx.close()
    if "ZK_GPROD_TREE_FUSE" not in os.environ:
        for fuse in ("1", "2", "3"):
            env = dict(os.environ, ZK_GPROD_TREE_FUSE=fuse)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--samples", str(a.samples), "--reps", str(a.reps), "--max-log",
                                str(a.max_log)], capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                raise SystemExit("child failed:\n" + r.stdout + r.stderr)
            lines += r.stdout.splitlines()
            print(r.stdout, end="", flush=True)
    if verdicts:
        wins = [v for v in verdicts if v[2] > v[3]]
        loses = [v for v in verdicts if -v[2] > v[3]]
        lines.append("the default of ZK_PERM_FUSE that follows: the fused route is faster by more than the spread at %d of %d shapes, slower by more "
                     "than the spread at %d: %s" % (len(wins), len(verdicts), len(loses), "1 (fused)" if len(wins) == len(verdicts) else "0 (unfused)"))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
