"""UnivariatePolynomial interpolation on the device: zk_upoly_interpolate and zk_upoly_interpolate_xy device time split into
weights, direct tree levels, NTT tree levels and block merges (zk_bench_upoly_interp: HIP events on the context's stream, the
average of --reps calls after one warm-up call), next to six zk_ntt calls of the top level's transform size measured in the same
run (zk_bench_ntt).  Output: profiles/upoly_interp.log (the kernel statistics come from a separate rocprofv3 run of --profile).

  python tools/upoly_interp_bench.py [--reps 3] [--out profiles/upoly_interp.log]
  python tools/upoly_interp_bench.py --profile     (two interpolations at 2^24: for rocprofv3 --kernel-trace --stats)

The direct / NTT crossover (ZK_UPOLY_INTERP_DIRECT_LOG = 7 or 8) runs in child processes."""
import argparse
import ctypes as c
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import zk_amd  # noqa: E402
from oracle import binding as orc  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402
from zk_amd import UnivariatePolynomial as UP  # noqa: E402
from zk_amd._lib import lib  # noqa: E402

FIELD = zk_amd.BN254_FR
INTERP = [1 << 12, 1 << 16, 1 << 20, (1 << 20) + (1 << 17) + 3, 1 << 24]
XY = [1 << 10, 1 << 12, 1 << 14, 1 << 16]
D_DEFAULT = int(os.environ.get("ZK_UPOLY_INTERP_DIRECT_LOG", "7"))


def bench(ctx, xs, ys, reps):
    out = (c.c_double * 5)()
    lib.zk_bench_upoly_interp(ctx._h, xs._h if xs is not None else None, ys._h, 1, out)   # warm-up: kernels loaded, plans built
    rc = lib.zk_bench_upoly_interp(ctx._h, xs._h if xs is not None else None, ys._h, reps, out)
    if rc:
        raise zk_amd.ZkError(rc)
    return list(out)


def ntt_ms(ctx, n):
    log_n = max(8, (n - 1).bit_length())
    t = MLE.random(ctx, log_n, 5)
    o = MLE.random(ctx, log_n, 6)
    return zk_amd.bench_ntt(ctx, t, o, False, reps=5), log_n


def run(reps, sizes_i, sizes_xy):
    ctx = zk_amd.Context(FIELD, 0)
    lines = []
    fmt = "{:<16} n={:>9}  total {:9.3f} ms  weights {:8.3f}  direct {:8.3f}  ntt-levels {:9.3f}  merges {:8.3f}{}"
    for n in sizes_i:
        ys = UP.new(ctx, orc.fill_random(FIELD, 11, n))
        r = bench(ctx, None, ys, reps)
        extra = ""
        if n & (n - 1) == 0 and n >= 1 << 12:
            t, log_n = ntt_ms(ctx, n)
            levels = log_n - D_DEFAULT   # every NTT level transforms n points six times
            extra = f"  | zk_ntt(2^{log_n}) {t:.3f} ms; per NTT level {r[3] / levels:.3f} ms = {r[3] / (levels * 6 * t):.2f} x six zk_ntt"
        lines.append(fmt.format("interpolate", n, *r, extra))
        ys.free()
    for n in sizes_xy:
        e1 = np.zeros((n, 4), dtype=np.uint64)
        e1[1] = orc.from_u64(FIELD, 1)
        xs = UP.new(ctx, zk_amd.fft(ctx, e1))
        ys = UP.new(ctx, orc.fill_random(FIELD, 12, n))
        r = bench(ctx, xs, ys, reps)
        rate = n * (n - 1) / (r[1] * 1e-3)
        lines.append(fmt.format("interpolate_xy", n, *r, f"  | weights {rate:.3g} modmul/s (n(n-1) differences)"))
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upoly_interp.log"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.profile:
        ctx = zk_amd.Context(FIELD, 0)
        ys = UP.new(ctx, orc.fill_random(FIELD, 11, 1 << 24))
        for _ in range(2):
            UP.interpolate(ctx, ys).free()
        ctx.close()
        return
    if a.child:
        print("\n".join(run(a.reps, [1 << 16, 1 << 20, 1 << 24], [])))
        return
    lines = ["# tools/upoly_interp_bench.py, BN254, MI355X; device ms, average of %d calls after a warm-up" % a.reps]
    lines += run(a.reps, INTERP, XY)
    for d in (7, 8):
        env = dict(os.environ, ZK_UPOLY_INTERP_DIRECT_LOG=str(d))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=env, capture_output=True,
                           text=True, timeout=600)
        lines.append(f"# crossover: ZK_UPOLY_INTERP_DIRECT_LOG={d} (exit {r.returncode})")
        lines += r.stdout.strip().splitlines()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
