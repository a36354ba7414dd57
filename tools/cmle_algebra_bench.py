"""Device times of the coefficient-form algebra (zk_bench_cmle_algebra) at 2^n, BN254, one box, beside the streaming-copy yardstick
(zk_bench_copy) of the same run.

  python3 tools/cmle_algebra_bench.py [--out profiles/cmle_algebra.log] [--n 24] [--reps 20] [--rounds 3]

Every line: device ms (HIP events around `reps` back-to-back calls, the median of `rounds` such windows taken in turn with the other
operations), the bytes the operation has to move (source read once + result written, in 32-byte elements; the passes partial_evaluate
makes after its first are included, they are part of the algorithm) and the rate those two give."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import DeviceCoeffMultilinear as DC  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402

F = zk_amd.BN254_FR


def pe_bytes(n, s):
    """source once, then every pass's output written and (but for the last) read again: groups of three from the top"""
    total, m, left = 32 << n, n, s
    while left:
        g = min(3, left)
        m, left = m - g, left - g
        total += (32 << m) * (2 if left else 1)
    return total


def box_state():
    """clocks and load of every GPU of the box as rocm-smi shows them (read only), one line"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showuse", "--csv"], capture_output=True, text=True, timeout=30)
        rows = [ln for ln in r.stdout.splitlines() if ln.strip()]
        return " | ".join(rows) if r.returncode == 0 and rows else "rocm-smi gave nothing"
    except (OSError, subprocess.TimeoutExpired) as e:
        return f"rocm-smi unavailable ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmle_algebra.log"))
    ap.add_argument("--n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    n = a.n
    before = box_state()
    ctx = zk_amd.Context(F, 0)
    p = DC.interpolate(ctx, MLE.random(ctx, n, 0xA16E))
    q = DC.interpolate(ctx, MLE.random(ctx, n, 0xA16F))
    half = n // 2
    ma = DC.interpolate(ctx, MLE.random(ctx, half, 0xA170))
    mb = DC.interpolate(ctx, MLE.random(ctx, n - half, 0xA171))
    val = lambda i: zk_amd.fe_from_ints(F, [(0x9E3779B97F4A7C15 * (i + 7)) ** 3])[0]  # noqa: E731
    sel = lambda v: [i == v for i in range(n)]  # noqa: E731
    sets = {"low3": [0, 1, 2], "high3": [n - 3, n - 2, n - 1], "mixed7": [0, 3, 7, n // 2, n // 2 + 3, n - 5, n - 1]}
    jobs = {}
    for name, vs in sets.items():
        asg = [(sel(v), val(v)) for v in vs]
        jobs[f"partial_evaluate_{name}"] = (lambda asg=asg: p.bench_algebra(0, assignments=asg, reps=a.reps), pe_bytes(n, len(vs)))
    jobs["add"] = (lambda: p.bench_algebra(1, other=q, reps=a.reps), 3 * (32 << n))
    jobs["scalar_multiply"] = (lambda: p.bench_algebra(2, scalar=val(1), reps=a.reps), 2 * (32 << n))
    jobs[f"mul_{half}x{n - half}"] = (lambda: ma.bench_algebra(3, other=mb, reps=a.reps), (32 << n) + (32 << half) + (32 << (n - half)))
    times = {k: [] for k in jobs}
    copies = []
    for _ in range(a.rounds):   # the operations in turn, the yardstick among them: a drift of the box shows in every line alike
        copies.append(ctx.bench_copy(32 << n, reps=a.reps))
        for k, (fn, _) in jobs.items():
            times[k].append(fn())
    copy_gbps = statistics.median(copies)
    after = box_state()
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# tools/cmle_algebra_bench.py on {torch.cuda.get_device_name(0)} ({prop.gcnArchName}, {prop.multi_processor_count} CUs, rocm {torch.version.hip}): "
             f"BN254, n={n}, device ms = median of {a.rounds} windows of {a.reps} back-to-back calls (HIP events)",
             f"# box before: {before}",
             f"# box after: {after}",
             f"zk_bench_copy size={32 << n} GBps={copy_gbps:.0f} (min {min(copies):.0f} max {max(copies):.0f}; read + write, as the hook counts them)"]
    for k, (_, nbytes) in jobs.items():
        ms = statistics.median(times[k])
        gbps = nbytes / (ms * 1e-3) / 1e9
        lines.append(f"{k} ms={ms:.4f} (min {min(times[k]):.4f} max {max(times[k]):.4f}) bytes={nbytes} GBps={gbps:.0f} of_copy={gbps / copy_gbps:.2f}")
    for line in lines:
        print(line, flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
