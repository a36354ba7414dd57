"""Batch inversion and running products on the device: zk_mle_batch_inverse on its default path and on each forced path, and
zk_mle_prefix_product (zk_bench_batch_inverse: HIP events on the context's stream, the average of --inner back-to-back calls after as
many untimed ones), --samples such measurements per line: median and minimum.  Two tables: both sides of the one-launch crossover
(ZK_BATCH_INV_ONE_LAUNCH_MAX) at 2^6 .. 2^11 elements, and 2^12, 2^16, 2^20, 2^24 elements beside zk_bench_copy of the same 96 bytes
per element and zk_bench_modmul from the same process, with the achieved share of each roof (bytes / copy rate; 4 multiplications per
element / multiplier rate).  The variants alternate inside one run and the box's load and clocks are logged before and after.
Output: profiles/batch_inverse.log.

  python tools/batch_inverse_bench.py [--samples 20] [--max-log 24] [--out profiles/batch_inverse.log]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402

FIELD = zk_amd.BN254_FR
DEFAULT, ONE, THREE, PREFIX = 0, 1, 2, 3
NAMES = {DEFAULT: "default", ONE: "one launch", THREE: "three launches", PREFIX: "prefix_product"}
BYTES_PER_ELEM = 96   # the three launches: two reads and one write of 32 bytes
MULS_PER_ELEM = 4.0   # counted from inv_kernels.cuh at kInvPerThread = 8: 1 (chunk products) + 3 (prefixes, tree, back-substitution)


def box_state(tag):
    lines = [f"# box {tag}: loadavg {' '.join('%.2f' % v for v in os.getloadavg())}"]
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showuse"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln or "use" in ln.lower())]
        lines += ["# box %s: %s" % (tag, ln) for ln in keep]
    except (OSError, subprocess.TimeoutExpired) as e:
        lines.append(f"# box {tag}: rocm-smi not available ({type(e).__name__})")
    return lines


def inner_reps(n_vars):
    return 20 if n_vars <= 16 else 5 if n_vars <= 20 else 3


def measure(t, out, paths, samples):
    """{path: (median ms, min ms)}; the paths alternate sample by sample"""
    got = {p: [] for p in paths}
    for p in paths:
        t.bench_batch_inverse(out, p, 2)   # warm: code objects, pool blocks
    for _ in range(samples):
        for p in paths:
            got[p].append(t.bench_batch_inverse(out, p, inner_reps(t.n_vars())))
    return {p: (statistics.median(v), min(v)) for p, v in got.items()}


def block_crossover(ctx, samples):
    lines = []
    for n_vars in range(6, 12):
        t, out = MLE.random(ctx, n_vars, 11), MLE.alloc(ctx, n_vars)
        try:
            r = measure(t, out, (ONE, THREE), samples)
        except zk_amd.ZkError as e:   # more than one chunk: there is no one-launch side
            lines.append(f"crossover n=2^{n_vars:<2}  one launch not available ({e})")
            continue
        lines.append(f"crossover n=2^{n_vars:<2}  one launch median {r[ONE][0] * 1e3:8.2f} us min {r[ONE][1] * 1e3:8.2f} us  | three launches median "
                     f"{r[THREE][0] * 1e3:8.2f} us min {r[THREE][1] * 1e3:8.2f} us  | three / one {r[THREE][0] / r[ONE][0]:.3f}")
        t.free()
        out.free()
    return lines


def block_sizes(ctx, samples, max_log):
    lines = []
    modmul = statistics.median(ctx.bench_modmul() for _ in range(5))
    lines.append(f"zk_bench_modmul (fe_mul chain, this process): {modmul:.4g} modmul/s")
    for n_vars in (12, 16, 20, 24):
        if n_vars > max_log:
            continue
        n = 1 << n_vars
        t, out = MLE.random(ctx, n_vars, 13), MLE.alloc(ctx, n_vars)
        r = measure(t, out, (DEFAULT, THREE, PREFIX), samples)
        nbytes = BYTES_PER_ELEM * n
        gbps = statistics.median(ctx.bench_copy(max(nbytes // 2, 16), 10) for _ in range(5))   # the hook moves `bytes` in and `bytes` out
        copy_ms = nbytes / (gbps * 1e9) * 1e3
        mul_ms = MULS_PER_ELEM * n / modmul * 1e3
        for p in (DEFAULT, THREE, PREFIX):
            med, lo = r[p]
            line = f"n=2^{n_vars:<2} {NAMES[p]:<15} median {med:9.4f} ms  min {lo:9.4f} ms  {n / (med * 1e-3) / 1e9:7.3f} Gelem/s"
            if p != PREFIX:
                line += (f"  | copy of the same {BYTES_PER_ELEM} B/elem {copy_ms:8.4f} ms ({gbps / 1e3:.2f} TB/s): {copy_ms / med:6.1%} of the bandwidth roof"
                         f"  | {MULS_PER_ELEM:.0f} mul/elem at the modmul rate {mul_ms:8.4f} ms: {mul_ms / med:6.1%} of the multiplier roof")
            lines.append(line)
        t.free()
        out.free()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_inverse.log"))
    a = ap.parse_args()
    lines = ["# tools/batch_inverse_bench.py, BN254, MI355X; device ms between HIP events per call (average of 20 / 5 / 3 back-to-back calls at "
             "<= 2^16 / <= 2^20 / 2^24 after as many untimed ones); median and minimum of %d such samples" % a.samples]
    lines += box_state("before")
    ctx = zk_amd.Context(FIELD, 0)
    for block in (lambda: block_crossover(ctx, a.samples), lambda: block_sizes(ctx, a.samples, a.max_log)):
        lines += block()
        print("\n".join(lines[-16:]), flush=True)
    ctx.close()
    lines += box_state("after")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
