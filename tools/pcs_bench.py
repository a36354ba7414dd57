"""The FRI polynomial commitment on the device, BN254.  zk_deep_quotient (zk_bench_deep_quotient: HIP events on the context's stream, the
average of back-to-back quotients after as many untimed ones; the power table and the pointer array are made outside the timed loop) at
2^20 and 2^24 points over k = 1, 4, 16 columns; --samples such measurements per line: median and minimum.  Beside each, from the same
process: zk_bench_copy of the bytes it must move ((k + 1) 32 per row: the roof for bytes) and the multiplier roof: the multiplications
counted from pcs_kernels.cuh (k + 6 per output above 2^12 points, plus about 0.5 for the LDS product trees) against zk_bench_modmul's
carry-free rate.  At small sizes the quotient against its own lone inversion (one chunk: one launch).  The unfused comparison:
zk_mle_batch_inverse of a materialised table of the same length plus a copy of the column and output traffic a separate combine pass
would move ((k + 2) 32 per row).  Then zk_pcs_commit and zk_pcs_open by wall clock at d = 20, b = 2, a = 3, f = 2, Q = 32, k = 1 and 4,
beside zk_fri_prove of the same shape, with the parts of an opening timed on their own through the public calls.
Output: profiles/pcs.log (--append adds a run to the log).

  python tools/pcs_bench.py [--samples 5] [--max-log 24] [--append] [--out profiles/pcs.log]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MerkleTree  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402
from zk_amd import UnivariatePolynomial as Poly  # noqa: E402

FIELD = zk_amd.BN254_FR
MULS_PER_OUTPUT_TREES = 0.5   # 255 / 2048 in launch 1 and 3 * 255 / 2048 in launch 3 (pcs_kernels.cuh)


def muls_per_output(k, n_vars):
    """multiplications per output, counted from pcs_kernels.cuh: above one chunk 2 (launch 1) + k + 4 (launch 3), less the two power
    table composes up to 2^12 points; one chunk: launch 3 alone"""
    if n_vars <= 11:
        return k + 3 + 3 * 255 / 2048
    return k + 6 - (2 if n_vars <= 12 else 0) + MULS_PER_OUTPUT_TREES


def inner_reps(n_vars):
    return 20 if n_vars <= 20 else 3


def median_of(fn, samples):
    got = [fn() for _ in range(samples)]
    return statistics.median(got), min(got)


def block_quotient(ctx, samples, max_log):
    lines = []
    modmul = statistics.median(ctx.bench_modmul(2000, 1) for _ in range(3))
    lines.append(f"zk_bench_modmul, carry-free multiplier (variant 1): {modmul / 1e9:.1f} G modmul/s")
    for n_vars in (8, 11, 12, 16):   # the lone inversion at small sizes: one launch up to 2^11 points
        cols = [MLE.random(ctx, n_vars, 61)]
        out = MLE.alloc(ctx, n_vars)
        zk_amd.bench_deep_quotient(cols, out, 1)
        med, lo = median_of(lambda: zk_amd.bench_deep_quotient(cols, out, 50), samples)
        inv_med, _ = median_of(lambda: cols[0].bench_batch_inverse(out, 0, 50), samples)
        lines.append(f"n=2^{n_vars} k=1 zk_deep_quotient median {med * 1e3:8.2f} us  min {lo * 1e3:8.2f} us | zk_mle_batch_inverse of as many elements "
                     f"(the same lone fe_inverse_binary) {inv_med * 1e3:8.2f} us")
        out.free()
        cols[0].free()
    for n_vars in (20, 24):
        if n_vars > max_log:
            continue
        n = 1 << n_vars
        out = MLE.alloc(ctx, n_vars)
        cols = []
        for k in (1, 4, 16):
            while len(cols) < k:
                cols.append(MLE.random(ctx, n_vars, 70 + len(cols)))
            zk_amd.bench_deep_quotient(cols, out, 1)   # warm: code objects, pool blocks
            med, lo = median_of(lambda: zk_amd.bench_deep_quotient(cols, out, inner_reps(n_vars)), samples)
            nbytes = 32 * (k + 1) * n
            gbps = statistics.median(ctx.bench_copy(nbytes // 2, 5) for _ in range(3))   # the hook moves `bytes` in and `bytes` out
            copy_ms = nbytes / (gbps * 1e9) * 1e3
            muls = muls_per_output(k, n_vars) * n
            mul_ms = muls / modmul * 1e3
            lines.append(f"n=2^{n_vars} k={k:<2} zk_deep_quotient median {med:8.4f} ms  min {lo:8.4f} ms | copy of the same {nbytes / 2**20:7.1f} MiB {copy_ms:7.4f} ms "
                         f"({gbps / 1e3:.2f} TB/s): {copy_ms / med:6.1%} of the copy roof | {muls / 2**20:7.2f} Mi multiplications {mul_ms:7.4f} ms: "
                         f"{mul_ms / med:6.1%} of the multiplier roof")
            # unfused: the inverses of a materialised denominator table, then a combine pass that reads k columns and the inverses and writes q
            inv_med, _ = median_of(lambda: cols[0].bench_batch_inverse(out, 0, inner_reps(n_vars)), samples)
            comb_bytes = 32 * (k + 2) * n
            comb_gbps = statistics.median(ctx.bench_copy(comb_bytes // 2, 5) for _ in range(3))
            comb_ms = comb_bytes / (comb_gbps * 1e9) * 1e3
            lines.append(f"n=2^{n_vars} k={k:<2} unfused: zk_mle_batch_inverse of a materialised table {inv_med:8.4f} ms + a copy of the combine pass's "
                         f"{comb_bytes / 2**20:7.1f} MiB {comb_ms:7.4f} ms = {inv_med + comb_ms:8.4f} ms (writing the denominators not counted): fused / unfused "
                         f"{med / (inv_med + comb_ms):.3f}")
        for t in cols + [out]:
            t.free()
    return lines


def wall(fn, samples):
    fn()
    times = []
    for _ in range(samples):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def block_open(ctx, samples, max_log):
    d, b, a, f, q = (20, 2, 3, 2, 32) if max_log >= 22 else (max_log - 2 - (max_log - 4) % 3, 2, 3, 2, 32)
    shift = zk_amd.fe_from_int(FIELD, 5)
    z = zk_amd.fe_from_int(FIELD, 0x5EED)
    seed = bytes(range(32))
    lines = []
    polys = [Poly.new(ctx, MLE.random(ctx, d, 80 + c).evaluation_slice()) for c in range(4)]
    med, lo = wall(lambda: zk_amd.fri_prove(polys[0], d, b, a, f, q, shift, seed), samples)
    lines.append(f"zk_fri_prove d={d} b={b} a={a} f={f} Q={q} (one polynomial, its LDE included), wall clock: median {med:.3f} ms  min {lo:.3f} ms")

    def sync(x):
        ctx.synchronize()
        return x

    for k in (1, 4):
        lines.append(f"k={k} d={d} b={b} a={a} f={f} Q={q} ({zk_amd.pcs_proof_bytes(k, d, b, a, f, q)} proof bytes), wall clock:")
        med, lo = wall(lambda: sync(zk_amd.PolyCommitment.commit(polys[:k], d, b, a, shift)).free(), samples)
        lines.append(f"  zk_pcs_commit ({k} LDEs to 2^{d + b} points, the tree over {k << a} columns of 2^{d + b - a} rows; waited for): median {med:.3f} ms  min {lo:.3f} ms")
        com = zk_amd.PolyCommitment.commit(polys[:k], d, b, a, shift)
        med, lo = wall(lambda: com.open(z, f, q, seed), samples)
        lines.append(f"  zk_pcs_open (values, quotient, the FRI rounds, all openings): median {med:.3f} ms  min {lo:.3f} ms")
        com.free()
        # the parts on their own, through the public calls
        med, lo = wall(lambda: [p.evaluate(z) for p in polys[:k]], samples)
        lines.append(f"  values: {k} zk_upoly_evaluate calls, a wait each (the opening itself: two launches for all, one wait): median {med:.3f} ms  min {lo:.3f} ms")
        ldes = [zk_amd.fri_lde(p, d + b, shift) for p in polys[:k]]
        out = MLE.alloc(ctx, d + b)
        ms, _ = median_of(lambda: zk_amd.bench_deep_quotient(ldes, out, 5), samples)
        lines.append(f"  quotient: zk_deep_quotient of the {k} LDEs, device ms: median {ms:.3f} ms")
        med, lo = wall(lambda: sync(zk_amd.fri_lde(polys[0], d + b, shift)).free(), samples)
        lines.append(f"  FRI: zk_fri_prove above less its LDE ({med:.3f} ms) is what the opening runs on the quotient")
        m = d + b - a
        views = [t.partial_evaluate(0, zk_amd.fe_from_ints(FIELD, [(j >> (a - 1 - s)) & 1 for s in range(a)])) for t in ldes for j in range(1 << a)]
        tree = MerkleTree.commit(views)
        idx = [(0x9E3779B97F4A7C15 * (t + 1)) % (1 << m) for t in range(q)]
        med, lo = wall(lambda: tree.open(idx, views), samples)
        lines.append(f"  openings: {q} rows of the {k << a} column views through zk_merkle_open (a download and a wait of its own; the opening joins "
                     f"them to the prover's last): median {med:.3f} ms  min {lo:.3f} ms")
        tree.free()
        for t in views + ldes + [out]:
            t.free()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcs.log"))
    a = ap.parse_args()
    lines = ["# tools/pcs_bench.py, BN254, MI355X; quotients: device ms between HIP events per quotient (average of 20 / 3 back-to-back ones at 2^20 / 2^24 "
             "points, 50 at the small sizes, after as many untimed ones); median and minimum of %d such samples" % a.samples,
             "# loadavg %s" % " ".join("%.2f" % v for v in os.getloadavg())]
    ctx = zk_amd.Context(FIELD, 0)
    for block in (lambda: block_quotient(ctx, a.samples, a.max_log), lambda: block_open(ctx, a.samples, a.max_log)):
        lines += block()
        print("\n".join(lines[-24:]), flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "a" if a.append else "w").write(text)


if __name__ == "__main__":
    main()
