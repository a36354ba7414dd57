"""Sharding by index mod world: device time of zk_mle_split / zk_mle_interleave at n = 24 and the host wall clock of
zk_mle_upload_shard against zk_mle_upload of the same number of contiguous elements.  Output: profiles/shard_layout.log.

  python tools/shard_layout_bench.py [--reps 20]

split / interleave: each call is enqueued behind a spin kernel (torch.cuda._sleep) and bracketed by two torch events on the
context's stream (ctx.use_torch_stream()), so the host's own work in the call (handles, pool blocks, launch) is hidden and the
interval is the kernel's; median over --reps calls after warm-up.  Traffic counted: 2 * 2^24 * 32 B (every element read once and
written once).  zk_bench_copy (a plain 16-B-per-lane copy) is printed beside it as this device's copy ceiling.
upload_shard: wall clock around the whole call (it returns after the shard is on the device), median of --reps; against
zk_mle_upload of a contiguous 2^21-element array, the same bytes over the bus."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import zk_amd  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402

PEAK_TBS = 8.0


def device_us(ctx, fn, reps):
    """median device time (us) of fn() between two events, the host's enqueue hidden behind a spin kernel"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(2_000_000)   # ~1 ms of spinning: the call below is enqueued before the stream reaches e0
        e0.record()
        keep = fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
        del keep
    return float(np.median(out))


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        keep = fn()
        out.append((time.perf_counter() - t0) * 1e3)
        del keep
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=24)
    a = ap.parse_args()
    n = a.n
    ctx = zk_amd.Context(zk_amd.BN254_FR, 0)
    ctx.use_torch_stream()
    copy_gbps = ctx.bench_copy(32 << n, reps=20)
    traffic = 2.0 * (32 << n)
    print(f"device: {torch.cuda.get_device_name(0)}; n = {n}; traffic per call {traffic / 2**30:.2f} GiB; "
          f"zk_bench_copy {copy_gbps / 1e3:.2f} TB/s = {copy_gbps / 1e3 / PEAK_TBS:.3f} of {PEAK_TBS:.0f} TB/s")
    t = MLE.random(ctx, n, 1)
    rows = []
    for world in (2, 8, 64):
        shards = t.split(world)
        for _ in range(3):   # warm-up: code objects, pool blocks of both sizes
            MLE.interleave(t.split(world))
        us_split = device_us(ctx, lambda: t.split(world), a.reps)
        us_inter = device_us(ctx, lambda: MLE.interleave(shards), a.reps)
        for name, us in (("split", us_split), ("interleave", us_inter)):
            tbs = traffic / (us * 1e-6) / 1e12
            rows.append({"kernel": name, "world": world, "us": round(us, 1), "tb_s": round(tbs, 3), "of_8tbs": round(tbs / PEAK_TBS, 3),
                         "of_copy": round(tbs / (copy_gbps / 1e3), 3)})
            print(f"{name:>10}  W = {world:3d}: {us:8.1f} us  {tbs:5.2f} TB/s  {tbs / PEAK_TBS:.3f} of 8 TB/s  "
                  f"{tbs / (copy_gbps / 1e3):.3f} of zk_bench_copy")
        del shards
    # upload_shard (n, W = 8) against a contiguous upload of the same 2^(n-3) elements
    host = t.evaluation_slice()
    world, m = 8, n - 3
    contiguous = np.ascontiguousarray(host[: 1 << m])
    for _ in range(2):
        MLE.new_shard(ctx, n, host, world, 3)
        MLE.new(ctx, m, contiguous)
    ms_shard = wall_ms(lambda: MLE.new_shard(ctx, n, host, world, 3), a.reps)
    ms_contig = wall_ms(lambda: MLE.new(ctx, m, contiguous), a.reps)
    assert MLE.new_shard(ctx, n, host, world, 3) == t.split(world)[3]
    ratio = ms_shard / ms_contig
    print(f"upload_shard  n = {n}, W = {world}: {ms_shard:.2f} ms   zk_mle_upload of 2^{m} contiguous elements: {ms_contig:.2f} ms   "
          f"ratio {ratio:.2f} (target <= 1.5)")
    print(json.dumps({"n": n, "copy_tb_s": round(copy_gbps / 1e3, 3), "rows": rows, "upload_shard_ms": round(ms_shard, 2),
                      "upload_contiguous_ms": round(ms_contig, 2), "upload_ratio": round(ratio, 2)}))
    ctx.use_own_stream()


if __name__ == "__main__":
    main()
