"""Device times of the dense coefficient-form calls (zk_bench_cmle) beside the existing paths they mirror, BN254, one box.

  python3 tools/cmle_bench.py [--out profiles/cmle.log] [--sizes 16,20,22,24] [--reps 20]

interpolate / to_evaluation / evaluate: average device ms of `reps` back-to-back enqueues between two HIP events.  Beside them:
zk_mle_evaluate's device time at the same n (zk_bench_evaluate_device), zk_coeff_to_evaluation wall clock with 1024 terms and with
all 2^n terms (the host-to-device copy of the list included: it is part of that call), and the wall clock per call of both evaluates.
`--profile N` only runs interpolate N times at 2^24 (the rocprofv3 --pmc run)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zk_amd  # noqa: E402
from zk_amd import DeviceCoeffMultilinear as DC  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmle.log"))
    ap.add_argument("--sizes", default="16,20,22,24")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", type=int, default=0)
    a = ap.parse_args()
    ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
    if a.profile:
        t = MLE.random(ctx, 24, 1)
        for _ in range(a.profile):
            DC.interpolate(ctx, t).free()
        ctx.synchronize()
        return
    lines = ["# tools/cmle_bench.py: BN254, MI355X, device ms (HIP events, average of %d back-to-back calls) unless marked wall" % a.reps]
    for n in [int(x) for x in a.sizes.split(",")]:
        t = MLE.random(ctx, n, 0xC0DE + n)
        d = DC.interpolate(ctx, t)
        pt = zk_amd.fe_from_ints(zk_amd.BN254_FR, [(0x1234567 * (i + 3)) ** 5 for i in range(n)])
        pt_m1 = pt.copy()
        pt_m1[::4] = zk_amd.fe_from_ints(zk_amd.BN254_FR, [-1])   # every fourth coordinate -1: the fold path
        r = {
            "interpolate": d.bench(0, table=t, reps=a.reps),
            "to_evaluation": d.bench(1, reps=a.reps),
            "evaluate": d.bench(2, point=pt, reps=a.reps),
            "evaluate_minus1_quarter": d.bench(2, point=pt_m1, reps=a.reps),
            "mle_evaluate": zk_amd.bench_evaluate_device(t, pt, reps=a.reps),
        }
        r["evaluate_wall"] = wall_ms(lambda: d.evaluate_slice(pt), a.reps)
        r["mle_evaluate_wall"] = wall_ms(lambda: t.evaluate(pt), a.reps)
        co = d.coefficients()
        few = zk_amd.CoeffMultilinearPolynomial(zk_amd.BN254_FR, n, {k: co[k] for k in range(1024)})
        r["coeff_to_evaluation_1k_terms_wall"] = wall_ms(lambda: few.to_evaluation_form(ctx).free(), 5)
        dense = zk_amd.CoeffMultilinearPolynomial.__new__(zk_amd.CoeffMultilinearPolynomial)
        dense.field, dense._n_vars = zk_amd.BN254_FR, n
        dense._flat = (np.arange(1 << n, dtype=np.uint64), np.ascontiguousarray(co))   # a full 2^n-term list without a 2^n-entry dict
        r["coeff_to_evaluation_all_terms_wall"] = wall_ms(lambda: dense.to_evaluation_form(ctx).free(), 3)
        r["to_evaluation_wall"] = wall_ms(lambda: (d.to_evaluation_form().free(), ctx.synchronize()), 5)
        gib = (32 << n) / 2**30
        lines.append(f"n={n} " + " ".join(f"{k}={v:.4f}" for k, v in r.items()) +
                     f"  interpolate_GBps={3 * 2 * gib * 2**30 / (r['interpolate'] * 1e-3) / 1e9:.0f} (three crossings)"
                     f"  evaluate/mle_evaluate={r['evaluate'] / r['mle_evaluate']:.3f}")
        print(lines[-1], flush=True)
        d.free()
        t.free()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
