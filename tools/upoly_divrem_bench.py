"""UnivariatePolynomial division with remainder on the device: zk_upoly_divrem on its three paths (zk_bench_upoly_divrem: HIP events
on the context's stream, the average of --reps calls after a warm-up call; the Newton path split into series inverse, quotient
product and remainder).  Four tables: the direct kernel against Newton at la = 2 lb = 2^6 .. 2^11 (the default of
ZK_UPOLY_DIVREM_DIRECT_MAX), the linear-divisor scan against Newton at lb = 2, la = 2^12 .. 2^20, the scan at 2^20 and 2^24 beside
zk_bench_copy of the same 96 bytes per coefficient and zk_upoly_evaluate of the same polynomial, and Newton at la = 2 lb =
2^12 .. 2^24 beside zk_upoly_evaluate_many of the same N.  The compared variants alternate inside one run, every block runs twice, and
the box's load and clocks are logged before and after.  Output: profiles/upoly_divrem.log.

  python tools/upoly_divrem_bench.py [--reps 3] [--max-log 24] [--out profiles/upoly_divrem.log]"""
import argparse
import ctypes as c
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from oracle import binding as orc  # noqa: E402
from zk_amd import UnivariatePolynomial as UP  # noqa: E402
from zk_amd._lib import lib  # noqa: E402

FIELD = zk_amd.BN254_FR
DIRECT, LINEAR, NEWTON = 1, 2, 3


def box_state(tag):
    lines = [f"# box {tag}: loadavg {' '.join('%.2f' % v for v in os.getloadavg())}"]
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showuse"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln or "use" in ln.lower())]
        lines += ["# box %s: %s" % (tag, ln) for ln in keep]
    except (OSError, subprocess.TimeoutExpired) as e:
        lines.append(f"# box {tag}: rocm-smi not available ({type(e).__name__})")
    return lines


def divrem_ms(ctx, a, b, path, reps):
    out = (c.c_double * 4)()
    rc = lib.zk_bench_upoly_divrem(ctx._h, a._h, b._h, path, reps, out)
    if rc:
        raise zk_amd.ZkError(rc)
    return list(out)


def operands(ctx, la, lb, seed):
    return UP.new(ctx, orc.fill_random(FIELD, seed, la)), UP.new(ctx, orc.fill_random(FIELD, seed + 1, lb))   # a random leading coefficient: not zero


def split(r):
    return f"inverse {r[1]:8.3f}  quotient {r[2]:8.3f}  remainder {r[3]:8.3f}"


def block_direct(ctx, reps):
    lines = []
    for lg in range(6, 12):
        a, b = operands(ctx, 1 << lg, 1 << (lg - 1), 31)
        for rnd in (1, 2):
            d, n = divrem_ms(ctx, a, b, DIRECT, reps), divrem_ms(ctx, a, b, NEWTON, reps)
            lines.append(f"direct vs newton la=2^{lg:<2} lb=2^{lg - 1:<2} pass {rnd}  direct {d[0]:8.4f} ms  newton {n[0]:8.4f} ms ({split(n)})  direct / newton {d[0] / n[0]:.2f}")
        a.free()
        b.free()
    return lines


def block_linear(ctx, reps, max_log):
    lines = []
    for lg in range(12, min(20, max_log) + 1, 2):
        a, b = operands(ctx, 1 << lg, 2, 33)
        for rnd in (1, 2):
            s, n = divrem_ms(ctx, a, b, LINEAR, reps), divrem_ms(ctx, a, b, NEWTON, reps)
            lines.append(f"linear vs newton la=2^{lg:<2} lb=2 pass {rnd}  scan {s[0]:8.4f} ms  newton {n[0]:8.4f} ms ({split(n)})  newton / scan {n[0] / s[0]:.2f}")
        a.free()
        b.free()
    return lines


def block_linear_roofline(ctx, reps, max_log):
    lines = []
    for lg in sorted({min(20, max_log), min(24, max_log)}):
        la = 1 << lg
        a, b = operands(ctx, la, 2, 35)
        x = orc.fill_random(FIELD, 36, 1)[0]
        nbytes = 96 * la   # a read twice, q written once
        for rnd in (1, 2):
            s = divrem_ms(ctx, a, b, LINEAR, reps)
            gbps = ctx.bench_copy(nbytes // 2, reps)   # the hook moves `bytes` in and `bytes` out
            copy_ms = nbytes / (gbps * 1e9) * 1e3
            a.evaluate(x)
            t0 = time.perf_counter()
            for _ in range(reps):
                a.evaluate(x)
            ev_ms = (time.perf_counter() - t0) / reps * 1e3
            lines.append(f"linear la=2^{lg:<2} pass {rnd}  scan {s[0]:8.4f} ms = {nbytes / (s[0] * 1e-3) / 1e12:.2f} TB/s of its 96 B/coefficient  | zk_bench_copy of the same bytes "
                         f"{copy_ms:8.4f} ms ({gbps / 1e3:.2f} TB/s), scan / copy {s[0] / copy_ms:.2f}  | zk_upoly_evaluate (one read, host wait included) {ev_ms:8.4f} ms, "
                         f"scan / evaluate {s[0] / ev_ms:.2f}")
        a.free()
        b.free()
    return lines


def block_newton(ctx, reps, max_log):
    lines = []
    for lg in range(12, max_log + 1, 4):
        la = 1 << lg
        a, b = operands(ctx, la, la // 2, 37)
        xs = UP.new(ctx, orc.fill_random(FIELD, 39, la))
        em = (c.c_double * 6)()
        for rnd in (1, 2):
            n = divrem_ms(ctx, a, b, NEWTON, reps)
            rc = lib.zk_bench_upoly_evaluate_many(ctx._h, a._h, xs._h, 0, reps, em)
            if rc:
                raise zk_amd.ZkError(rc)
            lines.append(f"newton la=2^{lg:<2} lb=2^{lg - 1:<2} pass {rnd}  total {n[0]:9.3f} ms  {split(n)}  | evaluate_many n=L=2^{lg} {em[0]:9.3f} ms, ratio {n[0] / em[0]:.2f}")
        for h in (a, b, xs):
            h.free()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upoly_divrem.log"))
    a = ap.parse_args()
    lines = ["# tools/upoly_divrem_bench.py, BN254, MI355X; device ms between HIP events, average of %d calls after a warm-up call" % a.reps]
    lines += box_state("before")
    ctx = zk_amd.Context(FIELD, 0)
    for block in (lambda: block_direct(ctx, a.reps), lambda: block_linear(ctx, a.reps, a.max_log), lambda: block_linear_roofline(ctx, a.reps, a.max_log),
                  lambda: block_newton(ctx, a.reps, a.max_log)):
        lines += block()
        print("\n".join(lines[-12:]), flush=True)
    ctx.close()
    lines += box_state("after")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
