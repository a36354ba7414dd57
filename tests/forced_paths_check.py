"""Run by tests/test_gpu_forced_paths.py in child processes (the library reads its ZK_* switches once per process).

  ntt     under ZK_NTT_FULL_TABLE_MAX_LOG: zk_ntt forward and inverse at lg = 8, 9, 12, 13, 16, 17, 20, one fused-NTT product, one
          interpolation above the direct tree levels and one sharded transform (world 2 on one GPU), all three fields, each against
          the oracle its neighbouring test uses (orc.ntt_fast, the oracle composition of the product, the Lagrange restatement)
  interp  under ZK_UPOLY_INTERP_DIRECT_LOG: prints a digest of the interpolated coefficients at the small sizes and at 2^16 +- 1,
          for the parent to compare between settings"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import zk_amd  # noqa: E402
from oracle import binding as orc  # noqa: E402
from zk_amd import MultiLinearPolynomial as MLE  # noqa: E402
from zk_amd import UnivariatePolynomial as UP  # noqa: E402

FIELDS = (zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)
NTT_LOGS = (8, 9, 12, 13, 16, 17, 20)


def ntt_plan(log_n):
    """the pass radices of ntt_make_plan (ntt.hip) and the table size log2(R_p * I_p) of every pass but the last"""
    n_pass = max(2, (log_n + 7) // 8)
    base, rem = divmod(log_n, n_pass)
    radices = [base + (1 if p < rem else 0) for p in range(n_pass)]
    entries, done = [], 0
    for p in range(n_pass - 1):
        entries.append(log_n - done)
        done += radices[p]
    return radices, entries


def oracle_product(field, a, b):
    lc = a.shape[0] + b.shape[0] - 1
    n = 1 << (lc - 1).bit_length()
    pa, pb = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    pa[:a.shape[0]], pb[:b.shape[0]] = a, b
    prod = orc.prod_reduce(field, n.bit_length() - 1, [orc.ntt_fast(field, pa), orc.ntt_fast(field, pb)])
    return orc.ntt_fast(field, prod, inverse=True)[:lc]


def check_ntt():
    import torch

    from interp_ref import lagrange
    from zk_amd.distributed import GpuNttBackend, shard_of, sliced_shard_of

    max_log = int(os.environ["ZK_NTT_FULL_TABLE_MAX_LOG"])
    for lg in NTT_LOGS:
        radices, entries = ntt_plan(lg)
        print(f"plan lg={lg}: radices {radices}; middle-pass twiddles: "
              + ", ".join(f"pass {p}: 2^{e} {'table' if e <= max_log else 'composed'}" for p, e in enumerate(entries)))
    checked = 0
    for field in FIELDS:
        ctx = zk_amd.Context(field, 0)
        for lg in NTT_LOGS:
            v = orc.fill_random(field, 4100 + lg, 1 << lg)
            f = zk_amd.fft(ctx, v)
            assert np.array_equal(f, orc.ntt_fast(field, v)), ("fft", field, lg)
            assert np.array_equal(zk_amd.ifft(ctx, f), v), ("ifft", field, lg)
            checked += 2
        # fused-NTT product (pad-load first pass, multiply-store and truncating last passes): N = 2^17, uneven operands
        a, b = orc.fill_random(field, 4200, (1 << 16) - 37), orc.fill_random(field, 4201, (1 << 16) - 1000)
        assert np.array_equal((UP.new(ctx, a) * UP.new(ctx, b)).coefficients(), oracle_product(field, a, b)), ("upoly_mul", field)
        # interpolation above the direct tree levels (batched NTT passes) against the Lagrange restatement
        n = 513
        ys = orc.fill_random(field, 4300, n)
        assert orc.to_ints(field, UP.interpolate(ctx, ys).coefficients()) == lagrange(list(range(n)), orc.to_ints(field, ys), orc.modulus(field)), (
            "interpolate", field)
        # sharded transform, world 2 on one GPU, the exchange done by hand (as tests/test_gpu_shard.py does)
        world, log_n = 2, 18
        x = orc.fill_random(field, 4400, 1 << log_n)
        X = orc.ntt_fast(field, x, False)
        fw = [GpuNttBackend(MLE.new(ctx, log_n - 1, shard_of(x, r, world)), r, world) for r in range(world)]
        for bk in fw:
            bk.local_ntt(False)
            bk.twiddle(False)
        sends = [bk.send_tensor().view(world, -1) for bk in fw]
        for s, bk in enumerate(fw):
            bk.recv_tensor().view(world, -1).copy_(torch.stack([sends[r][s] for r in range(world)]))
        for r, bk in enumerate(fw):
            bk.across(False)
            assert np.array_equal(bk.result().evaluation_slice(), sliced_shard_of(X, r, world)), ("sharded ntt", field, r)
        checked += 3
        ctx.close()
    print(f"forced ntt ok: {checked} checks bit-exact (ZK_NTT_FULL_TABLE_MAX_LOG={max_log})")


def check_interp():
    for field in FIELDS:
        ctx = zk_amd.Context(field, 0)
        for n in list(range(0, 41)) + [127, 128, 129, 255, 256, 257, 383, 384, 385, 513, (1 << 16) - 1, (1 << 16) + 1]:
            ys = orc.fill_random(field, 100 + n, n) if n else np.zeros((0, 4), dtype=np.uint64)
            got = UP.interpolate(ctx, ys).coefficients()
            print("DIGEST", field, n, hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest())
        ctx.close()
    print(f"forced interp ok (ZK_UPOLY_INTERP_DIRECT_LOG={os.environ.get('ZK_UPOLY_INTERP_DIRECT_LOG')})")


if __name__ == "__main__":
    {"ntt": check_ntt, "interp": check_interp}[sys.argv[1]]()
