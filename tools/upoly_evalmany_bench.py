"""UnivariatePolynomial multipoint evaluation on the device: zk_upoly_evaluate_many on its tree and direct paths
(zk_bench_upoly_evaluate_many: HIP events on the context's stream, the average of --reps calls after a warm-up call, the tree path
split into up-sweep, series inversion, root vector, NTT levels of the down-sweep and bottom kernel) next to zk_upoly_interpolate of
the same size, the two lopsided shapes, and zk_upoly_interpolate_xy with its weights from either path.  The compared variants
alternate inside one run, every block runs twice (the spread between the two passes is what a difference has to beat), and the
box's load and clocks are logged before and after.  Output: profiles/upoly_evalmany.log.

  python tools/upoly_evalmany_bench.py [--reps 3] [--max-log 24] [--out profiles/upoly_evalmany.log]

ZK_UPOLY_INTERP_XY_TREE_MIN is read once per process, so the interpolate_xy block runs in child processes (1: the weights from the
tree path, 2^40: the O(nx m) kernel the parent commit ran)."""
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
from zk_amd import UnivariatePolynomial as UP  # noqa: E402
from zk_amd._lib import lib  # noqa: E402

FIELD = zk_amd.BN254_FR
DIRECT_MAX_LOG = 18
XY_LOGS = (10, 12, 14, 16)
STAGES = ("up-sweep", "inversion", "root", "down-ntt", "bottom")


def box_state(tag):
    lines = [f"# box {tag}: loadavg {' '.join('%.2f' % v for v in os.getloadavg())}"]
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showuse"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln or "use" in ln.lower())]
        lines += ["# box %s: %s" % (tag, ln) for ln in keep]
    except (OSError, subprocess.TimeoutExpired) as e:
        lines.append(f"# box {tag}: rocm-smi not available ({type(e).__name__})")
    return lines


def evalmany_ms(ctx, p, xs, path, reps):
    out = (c.c_double * 6)()
    rc = lib.zk_bench_upoly_evaluate_many(ctx._h, p._h, xs._h, path, reps, out)
    if rc:
        raise zk_amd.ZkError(rc)
    return list(out)


def interp_ms(ctx, xs, ys, reps):
    out = (c.c_double * 5)()
    lib.zk_bench_upoly_interp(ctx._h, xs._h if xs is not None else None, ys._h, 1, out)   # warm-up
    rc = lib.zk_bench_upoly_interp(ctx._h, xs._h if xs is not None else None, ys._h, reps, out)
    if rc:
        raise zk_amd.ZkError(rc)
    return list(out)


def split(r):
    return "  ".join(f"{name} {v:8.3f}" for name, v in zip(STAGES, r[1:]))


def block_square(ctx, reps, max_log):
    lines = []
    for lg in range(10, max_log + 1, 2):
        n = 1 << lg
        p = UP.new(ctx, orc.fill_random(FIELD, 21, n))
        xs = UP.new(ctx, orc.fill_random(FIELD, 22, n))
        for rnd in (1, 2):   # tree, interpolate, direct, in turn, twice
            t = evalmany_ms(ctx, p, xs, 2, reps)
            i = interp_ms(ctx, None, xs, reps)
            lines.append(f"evaluate_many tree   n=L=2^{lg:<2} pass {rnd}  total {t[0]:9.3f} ms  {split(t)}  | interpolate {i[0]:9.3f} ms, ratio {t[0] / i[0]:.2f}")
            if lg <= DIRECT_MAX_LOG:
                d = evalmany_ms(ctx, p, xs, 1, reps if lg < DIRECT_MAX_LOG else 1)
                lines.append(f"evaluate_many direct n=L=2^{lg:<2} pass {rnd}  total {d[0]:9.3f} ms  | {n * n / (d[0] * 1e-3):.3g} modmul/s, direct / tree {d[0] / t[0]:.2f}")
        m = evalmany_ms(ctx, p, xs, 0, 1)
        lines.append(f"evaluate_many model  n=L=2^{lg:<2} picks the {'tree' if m[1] > 0 else 'direct'} path")
        p.free()
        xs.free()
    return lines


def block_lopsided(ctx, reps, max_log):
    lines = []
    for lg_l, lg_n in ((min(24, max_log), 10), (10, min(20, max_log))):
        p = UP.new(ctx, orc.fill_random(FIELD, 23, 1 << lg_l))
        xs = UP.new(ctx, orc.fill_random(FIELD, 24, 1 << lg_n))
        for rnd in (1, 2):
            t = evalmany_ms(ctx, p, xs, 2, reps)
            d = evalmany_ms(ctx, p, xs, 1, reps)
            lines.append(f"lopsided L=2^{lg_l} n=2^{lg_n} pass {rnd}  tree (padded to 2^{max(lg_l, lg_n)}) {t[0]:9.3f} ms  direct {d[0]:9.3f} ms")
        m = evalmany_ms(ctx, p, xs, 0, 1)
        lines.append(f"lopsided L=2^{lg_l} n=2^{lg_n} the model picks the {'tree' if m[1] > 0 else 'direct'} path")
        p.free()
        xs.free()
    return lines


def xy_points(ctx, n):
    e1 = np.zeros((n, 4), dtype=np.uint64)
    e1[1] = orc.from_u64(FIELD, 1)
    return UP.new(ctx, zk_amd.fft(ctx, e1))   # omega^i: distinct


def child_xy(reps, logs):
    ctx = zk_amd.Context(FIELD, 0)
    for lg in logs:
        n = 1 << lg
        xs, ys = xy_points(ctx, n), UP.new(ctx, orc.fill_random(FIELD, 12, n))
        r = interp_ms(ctx, xs, ys, reps)
        print(f"XY {lg} {r[0]:.4f} {r[1]:.4f}")
        xs.free()
        ys.free()
    ctx.close()


def block_xy(reps, max_log):
    lines, res = [], {}
    big = min(20, max_log)
    for rnd in (1, 2):
        for name, val, logs in (("tree", "1", list(XY_LOGS) + [big]), ("kernel", str(1 << 40), list(XY_LOGS))):
            env = dict(os.environ, ZK_UPOLY_INTERP_XY_TREE_MIN=val)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-xy", ",".join(map(str, logs)), "--reps", str(reps)], env=env,
                               capture_output=True, text=True, timeout=900)
            if r.returncode:
                lines.append(f"# interpolate_xy child {name} pass {rnd}: exit {r.returncode} {r.stderr[-300:]!r}")
            for ln in r.stdout.splitlines():
                if ln.startswith("XY "):
                    _, lg, tot, w = ln.split()
                    res[(name, rnd, int(lg))] = (float(tot), float(w))
    for lg in list(XY_LOGS) + [big]:
        for rnd in (1, 2):
            t, k = res.get(("tree", rnd, lg)), res.get(("kernel", rnd, lg))
            if t and k:
                lines.append(f"interpolate_xy n=2^{lg:<2} pass {rnd}  weights by tree: total {t[0]:9.3f} ms (weights {t[1]:9.3f})  by kernel: total {k[0]:9.3f} ms "
                             f"(weights {k[1]:9.3f})  kernel / tree {k[0] / t[0]:.2f}")
            elif t:
                lines.append(f"interpolate_xy n=2^{lg:<2} pass {rnd}  weights by tree: total {t[0]:9.3f} ms (weights {t[1]:9.3f})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upoly_evalmany.log"))
    ap.add_argument("--child-xy", default=None)
    a = ap.parse_args()
    if a.child_xy is not None:
        child_xy(a.reps, [int(v) for v in a.child_xy.split(",")])
        return
    lines = ["# tools/upoly_evalmany_bench.py, BN254, MI355X; device ms between HIP events, average of %d calls after a warm-up call" % a.reps]
    lines += box_state("before")
    ctx = zk_amd.Context(FIELD, 0)
    lines += block_square(ctx, a.reps, a.max_log)
    lines += block_lopsided(ctx, a.reps, a.max_log)
    ctx.close()
    lines += block_xy(a.reps, a.max_log)
    lines += box_state("after")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
