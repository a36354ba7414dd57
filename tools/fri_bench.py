"""FRI on the device, BN254.  The fold by 2^a (zk_bench_fri_fold: HIP events on the context's stream, the average of --inner back-to-back
folds after as many untimed ones; the power table and the constants are made outside the timed loop) with the fused kernel and with a
binary launches, a = 1, 2, 3, at 2^20 and 2^24 inputs; --samples such measurements per line: median and minimum, the two paths
alternating.  Beside each: zk_bench_copy of the bytes the form must move (fused: N + N / 2^a elements; binary: 1.5 N + 0.75 N + ...)
from the same process as the roof for bytes; zk_bench_fold (the MSB fold, the a = 1 access pattern with one multiplication) of the same
table in the same run; and the multiplier roof: the multiplications counted from fri_kernels.cuh (per output 1 compose + 1 for beta / s + (a - 1) squarings
+ 2^a - 1 butterfly products + 2^a - 1 - a constant twiddles = 2 (2^a - 1) + 1; the halves are shifts) against zk_bench_modmul's
carry-free rate.  Then the whole zk_fri_prove by wall clock at d = 20, b = 2, a = 3, f = 2, Q = 32, and its pieces timed on their own
through the public calls: the LDE, the commits of every layer (eight column tables each), the folds, the openings.
Output: profiles/fri.log (--append adds a run to the log).

  python tools/fri_bench.py [--samples 5] [--max-log 24] [--append] [--out profiles/fri.log]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import MerkleTree  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402
from zk_amd import UnivariatePolynomial as Poly  # noqa: E402

FIELD = zk_amd.BN254_FR
FUSED, BINARY = 1, 2
NAMES = {FUSED: "fused", BINARY: "binary launches"}


def inner_reps(n_vars):
    return 20 if n_vars <= 20 else 3


def muls_per_output(a, fused):
    """multiplications per OUTPUT of a fold by 2^a, counted from fri_kernels.cuh"""
    if fused:
        return 2 * ((1 << a) - 1) + 1
    return sum(3 << (a - 1 - l) for l in range(a))   # level l has 2^(a-1-l) outputs of k_fri_fold<1> per final output, 3 products each


def elems_moved(n, a, fused):
    if fused:
        return n + (n >> a)
    return sum((n >> l) + (n >> (l + 1)) for l in range(a))


def block_fold(ctx, samples, max_log):
    lines = []
    modmul = statistics.median(ctx.bench_modmul(2000, 1) for _ in range(3))
    lines.append(f"zk_bench_modmul, carry-free multiplier (variant 1): {modmul / 1e9:.1f} G modmul/s")
    for n_vars in (20, 24):
        if n_vars > max_log:
            continue
        n = 1 << n_vars
        layer = MLE.random(ctx, n_vars, 41)
        r = zk_amd.fe_from_int(FIELD, 12345)
        half = MLE.alloc(ctx, n_vars - 1)
        msb = statistics.median(layer.bench_fold(r, half, inner_reps(n_vars)) for _ in range(samples))
        half.free()
        lines.append(f"n=2^{n_vars} zk_bench_fold (MSB fold, 1 multiplication per output, 1.5 N elements moved): median {msb:.4f} ms")
        for a in (1, 2, 3):
            out = MLE.alloc(ctx, n_vars - a)
            got = {p: [] for p in NAMES}
            for p in NAMES:
                zk_amd.bench_fri_fold(layer, a, out, p, 1)   # warm: code objects, pool blocks
            for _ in range(samples):
                for p in NAMES:
                    got[p].append(zk_amd.bench_fri_fold(layer, a, out, p, inner_reps(n_vars)))
            for p in NAMES:
                med, lo = statistics.median(got[p]), min(got[p])
                nbytes = 32 * elems_moved(n, a, p == FUSED)
                gbps = statistics.median(ctx.bench_copy(max(nbytes // 2, 16), 5) for _ in range(3))   # the hook moves `bytes` in and `bytes` out
                copy_ms = nbytes / (gbps * 1e9) * 1e3
                muls = muls_per_output(a, p == FUSED) * (n >> a)
                mul_ms = muls / modmul * 1e3
                lines.append(f"n=2^{n_vars} a={a} {NAMES[p]:<15} median {med:8.4f} ms  min {lo:8.4f} ms | copy of the same {nbytes / 2**20:7.1f} MiB {copy_ms:7.4f} ms "
                             f"({gbps / 1e3:.2f} TB/s): {copy_ms / med:6.1%} of the copy roof | {muls / 2**20:6.2f} Mi multiplications {mul_ms:7.4f} ms: "
                             f"{mul_ms / med:6.1%} of the multiplier roof")
            lines.append(f"n=2^{n_vars} a={a} fused / binary launches (medians) {statistics.median(got[FUSED]) / statistics.median(got[BINARY]):.3f}"
                         f"; fused / MSB fold {statistics.median(got[FUSED]) / msb:.3f}")
            out.free()
        layer.free()
    return lines


def wall(fn, samples):
    fn()
    times = []
    for _ in range(samples):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def block_prove(ctx, samples, max_log):
    d, b, a, f, q = (20, 2, 3, 2, 32) if max_log >= 22 else (max_log - 2 - (max_log - 4) % 3, 2, 3, 2, 32)
    rounds = (d - f) // a
    shift = zk_amd.fe_from_int(FIELD, 5)
    beta = zk_amd.fe_from_int(FIELD, 0xBE7A)
    seed = bytes(range(32))
    coeffs = MLE.random(ctx, d, 51).evaluation_slice()
    poly = Poly.new(ctx, coeffs)
    lines = [f"zk_fri_prove d={d} b={b} a={a} f={f} Q={q} ({rounds} rounds, {zk_amd.fri_proof_bytes(d, b, a, f, q)} proof bytes), wall clock, ZK_FRI_FUSED_FOLD="
             f"{os.environ.get('ZK_FRI_FUSED_FOLD', 'unset')}:"]
    med, lo = wall(lambda: zk_amd.fri_prove(poly, d, b, a, f, q, shift, seed), samples)
    lines.append(f"  whole proof (LDE, {rounds} commits with one host wait each, {rounds} folds, final coefficients, {rounds} gather launches, one download): median {med:.3f} ms  min {lo:.3f} ms")

    def sync(x):
        ctx.synchronize()
        return x

    med, lo = wall(lambda: sync(zk_amd.fri_lde(poly, d + b, shift)).free(), samples)
    lines.append(f"  LDE to 2^{d + b} points (pad, shift powers, forward NTT): median {med:.3f} ms  min {lo:.3f} ms")
    # the layers of this shape, made once; then the commits, the folds and the openings over them, each kind timed on its own
    layers = [zk_amd.fri_lde(poly, d + b, shift)]
    for r in range(rounds):
        layers.append(zk_amd.fri_fold(layers[-1], a, shift, beta))
    columns = []
    for r in range(rounds):
        m = d + b - a * r - a
        ev = layers[r].evaluation_slice()
        columns.append([MLE.new(ctx, m, np.ascontiguousarray(ev[j << m:(j + 1) << m])) for j in range(1 << a)])

    def commits():
        trees = [MerkleTree.commit(cols) for cols in columns]
        for t in trees:
            t.root()   # the prover waits for every root before it can fold
        return trees

    med, lo = wall(lambda: [t.free() for t in commits()], samples)
    lines.append(f"  commits of the {rounds} layers (2^{a} columns each, the root of each waited for): median {med:.3f} ms  min {lo:.3f} ms")

    def folds():
        for r in range(rounds):
            zk_amd.fri_fold(layers[r], a, shift, beta, layers[r + 1])
        ctx.synchronize()

    med, lo = wall(folds, samples)
    lines.append(f"  folds of the {rounds} layers (a power table per call included): median {med:.3f} ms  min {lo:.3f} ms")
    trees = commits()
    idx = [(0x9E3779B97F4A7C15 * (k + 1)) % (1 << (d + b - a)) for k in range(q)]

    def openings():
        for r in range(rounds):
            m = d + b - a * r - a
            trees[r].open([i % (1 << m) for i in idx], columns[r])

    med, lo = wall(openings, samples)
    lines.append(f"  openings of {q} rows in each of the {rounds} layers through zk_merkle_open (a download and a wait per layer; the prover does one of each): "
                 f"median {med:.3f} ms  min {lo:.3f} ms")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri.log"))
    a = ap.parse_args()
    lines = ["# tools/fri_bench.py, BN254, MI355X; folds: device ms between HIP events per fold (average of 20 / 3 back-to-back folds at 2^20 / 2^24 "
             "inputs after as many untimed ones); median and minimum of %d such samples, fused and binary alternating" % a.samples,
             "# loadavg %s" % " ".join("%.2f" % v for v in os.getloadavg())]
    ctx = zk_amd.Context(FIELD, 0)
    for block in (lambda: block_fold(ctx, a.samples, a.max_log), lambda: block_prove(ctx, a.samples, a.max_log)):
        lines += block()
        print("\n".join(lines[-24:]), flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "a" if a.append else "w").write(text)


if __name__ == "__main__":
    main()
