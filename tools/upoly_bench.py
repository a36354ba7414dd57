"""UnivariatePolynomial on the device: zk_upoly_mul against the unfused composition of the existing ABI, the direct / NTT crossover,
and zk_upoly_evaluate at 2^24.  Output: profiles/upoly.log (the kernel statistics come from a separate rocprofv3 run of --profile).

  python tools/upoly_bench.py [--reps 7] [--out profiles/upoly.log]
  python tools/upoly_bench.py --profile          (one warm-up product, then two products at 2^24: for rocprofv3 --kernel-trace --stats)

Device times: each call is enqueued behind a spin kernel (torch.cuda._sleep) and bracketed by two torch events on the context's
stream (ctx.use_torch_stream()), after 0.8 s of untimed products (the shader clock climbs for tens of ms after idle); median of
--reps.  Fused and unfused run alternately on the same seeded inputs, and their downloaded outputs are compared byte for byte.
  fused   : zk_upoly_mul (exact-length operands in, exact-length product out)
  unfused : zk_ntt(A padded), zk_ntt(B padded), zk_prod_reduce, inverse zk_ntt on MultiLinearPolynomial handles of N elements
End to end (host arrays in, host array out, wall clock): fused = 2 x zk_upoly_upload + mul + download; unfused = 2 padded
zk_mle_upload + the four calls + zk_mle_download + truncation.
The crossover runs in two child processes (ZK_UPOLY_DIRECT_MAX = 2^40: always direct, = 0: NTT from 2^8 points)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import zk_amd  # noqa: E402
from oracle import binding as orc  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402
from zk_amd import UnivariatePolynomial as UP  # noqa: E402

FIELD = zk_amd.BN254_FR
PEAK_TBS = 8.0
CROSS_MINS = [1, 4, 8, 16, 24, 32, 48, 64, 96, 128, 256]
CROSS_TOTALS = [1 << 10, 1 << 14, 1 << 18, 1 << 22]


def device_us(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(2_000_000)
        e0.record()
        keep = fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
        del keep
    return float(np.median(out))


def settle(fn, ms=800.0):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        fn()
        torch.cuda.synchronize()


def rand(seed, n):
    return orc.fill_random(FIELD, seed, n)


def unfused(ctx, pa, pb, log_n):
    """the composition a user builds from the existing ABI today, on padded N-element handles"""
    fa, fb = MLE.alloc(ctx, log_n), MLE.alloc(ctx, log_n)
    zk_amd.ntt(ctx, pa, fa)
    zk_amd.ntt(ctx, pb, fb)
    prod = zk_amd.ProductPoly.new([fa, fb]).prod_reduce_device()
    out = MLE.alloc(ctx, log_n)
    zk_amd.ntt(ctx, prod, out, inverse=True)
    return out


def padded(a, n):
    p = np.zeros((n, 4), dtype=np.uint64)
    p[:a.shape[0]] = a
    return p


def product_rows(ctx, shapes, reps, log):
    for la, lb in shapes:
        lc = la + lb - 1
        log_n = (lc - 1).bit_length()
        a, b = rand(11 + la, la), rand(13 + lb, lb)
        A, B = UP.new(ctx, a), UP.new(ctx, b)
        fused_out = (A * B).coefficients()
        pa, pb = MLE.new(ctx, log_n, padded(a, 1 << log_n)), MLE.new(ctx, log_n, padded(b, 1 << log_n))
        un_out = unfused(ctx, pa, pb, log_n).evaluation_slice()[:lc]
        same = fused_out.tobytes() == un_out.tobytes()
        settle(lambda: A * B)
        f_us, u_us = [], []
        for _ in range(3):   # alternate
            f_us.append(device_us(lambda: A * B, reps))
            u_us.append(device_us(lambda: unfused(ctx, pa, pb, log_n), reps))
        f, u = float(np.median(f_us)), float(np.median(u_us))

        def e2e_fused():
            return (UP.new(ctx, a) * UP.new(ctx, b)).coefficients()

        def e2e_unfused():
            return unfused(ctx, MLE.new(ctx, log_n, padded(a, 1 << log_n)), MLE.new(ctx, log_n, padded(b, 1 << log_n)), log_n).evaluation_slice()[:lc]

        wf, wu = [], []
        for _ in range(3):
            t = time.perf_counter()
            e2e_fused()
            wf.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            e2e_unfused()
            wu.append((time.perf_counter() - t) * 1e3)
        log(f"la={la:>9} lb={lb:>9} N=2^{log_n:<2} device fused {f:10.1f} us  unfused {u:10.1f} us  ratio {u / f:5.2f}   "
            f"end-to-end fused {np.median(wf):8.2f} ms  unfused {np.median(wu):8.2f} ms   outputs identical: {same}")
        if not same:
            raise SystemExit("fused and unfused outputs differ")


def crossover_child(reps):
    ctx = zk_amd.Context(FIELD, 0)
    ctx.use_torch_stream()
    rows = []
    warm = UP.new(ctx, rand(1, 1 << 12))
    settle(lambda: warm * warm)
    for total in CROSS_TOTALS:
        for m in CROSS_MINS:
            A, B = UP.new(ctx, rand(2, m)), UP.new(ctx, rand(3, total - m))
            A * B   # plans / tables
            rows.append({"min": m, "total": total, "us": device_us(lambda: A * B, reps)})
    print("ROWS " + json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upoly.log"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--crossover-child", action="store_true")
    args = ap.parse_args()
    if args.crossover_child:
        return crossover_child(args.reps)
    ctx = zk_amd.Context(FIELD, 0)
    ctx.use_torch_stream()
    if args.profile:
        A, B = UP.new(ctx, rand(5, 1 << 23)), UP.new(ctx, rand(6, 1 << 23))
        (A * B).free()   # builds the plans and twiddle tables
        torch.cuda.synchronize()
        for _ in range(2):
            (A * B).free()
        torch.cuda.synchronize()
        print("profile: 1 warm-up + 2 products at la = lb = 2^23 (N = 2^24)")
        return
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# tools/upoly_bench.py on {torch.cuda.get_device_name(0)}, field bn254_fr, median of {args.reps} event-bracketed calls x 3 alternations")
    log("## zk_upoly_mul vs the unfused composition (zk_ntt x2, zk_prod_reduce, inverse zk_ntt on padded handles)")
    shapes = [(1 << k, 1 << k) for k in range(10, 24)] + [(1, 1 << 16), (3, 1 << 20), (40, 1 << 20), (100, 1 << 22), (1 << 12, 1 << 22)]
    product_rows(ctx, shapes, args.reps, log)
    log("## crossover: device us of the direct kernel (ZK_UPOLY_DIRECT_MAX=2^40) / the NTT path (=0), by min(la, lb) and la + lb")
    res = {}
    for name, val in (("direct", str(1 << 40)), ("ntt", "0")):
        env = dict(os.environ, ZK_UPOLY_DIRECT_MAX=val)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--crossover-child", "--reps", str(args.reps)], env=env,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stdout + r.stderr)
        res[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")][0][5:])
    for total in CROSS_TOTALS:
        cells, last_direct = [], 0
        for d, n in zip(res["direct"], res["ntt"]):
            if d["total"] != total:
                continue
            cells.append(f"{d['min']}: {d['us']:.0f}/{n['us']:.0f}")
            if d["us"] <= n["us"]:
                last_direct = d["min"]
        log(f"la+lb=2^{total.bit_length() - 1:<2} " + "  ".join(cells) + f"   -> direct no slower up to min = {last_direct}")
    log("## zk_upoly_evaluate at 2^24 (device time of the three launches; bytes = 2^24 x 32 B of coefficients read once)")
    h = UP.new(ctx, rand(7, 1 << 24))
    x = rand(8, 1)[0]
    settle(lambda: h.evaluate(x), 300)
    lib, cc = zk_amd._lib.lib, zk_amd._lib.c
    out = np.zeros(4, dtype=np.uint64)
    xp, op = x.ctypes.data_as(cc.POINTER(cc.c_uint64)), out.ctypes.data_as(cc.POINTER(cc.c_uint64))
    us = device_us(lambda: lib.zk_upoly_evaluate(ctx._h, h._h, xp, op), args.reps)
    tbs = (32 << 24) / (us * 1e-6) / 1e12
    log(f"evaluate 2^24: {us:.1f} us (includes the one host wait) = {tbs:.2f} TB/s = {tbs / PEAK_TBS:.2f} of {PEAK_TBS} TB/s")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
