"""check_fft_cases, the comparison tests/test_gpu_ntt_structured.py makes for every input of tests/ntt_vectors.py; and, run as a
script by that test in a child process under ZK_NTT_FULL_TABLE_MAX_LOG=0 (the library reads its ZK_* switches once per process):
the antiperiodic and constant inputs at 2^13 (two passes) and 2^17 (three) on BLS12-381."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import zk_amd  # noqa: E402
from oracle import binding as orc  # noqa: E402

import ntt_vectors as nv  # noqa: E402


def check_fft_cases(ctx, field, lg, cases):
    """zk_amd.fft against the oracle and the closed form, zk_amd.ifft of the expected spectrum giving x back, and the round trip;
    -> the number of cases"""
    cases = list(cases)
    with ThreadPoolExecutor(8) as ex:   # the oracle call releases the GIL
        oracle = list(ex.map(lambda case: orc.ntt_fast(field, case.x), cases))
    for case, want in zip(cases, oracle):
        tag = (field, lg, case.name)
        got = zk_amd.fft(ctx, case.x)
        assert np.array_equal(got, want), ("fft against the oracle", tag)
        if case.X is not None:
            assert np.array_equal(got, case.X), ("fft against the closed form", tag)
        if case.zeros is not None:
            assert not got[case.zeros].any(), ("outputs that are exactly 0", tag)
        # the inverse on the expected spectrum (mostly exact zeros where the family is sparse), then on the device's own output
        assert np.array_equal(zk_amd.ifft(ctx, want if case.X is None else case.X), case.x), ("ifft of the expected spectrum", tag)
        assert np.array_equal(zk_amd.ifft(ctx, got), case.x), ("round trip", tag)
    return len(cases)


if __name__ == "__main__":
    field = zk_amd.BLS12_381_FR
    ctx = zk_amd.Context(field, 0)
    try:
        done = sum(check_fft_cases(ctx, field, lg, nv.cases(field, lg, ("antiperiodic", "constant"))) for lg in (13, 17))
    finally:
        ctx.close()
    print(f"structured ntt ok: {done} cases (ZK_NTT_FULL_TABLE_MAX_LOG={os.environ.get('ZK_NTT_FULL_TABLE_MAX_LOG')})")
