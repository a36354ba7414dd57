"""Run by tests/test_gpu_batch_inverse.py in child processes (the library reads its ZK_* switches once per process), and imported by
it for the settings, so that the parent and the children hold the same cases.

  python batch_inverse_check.py <setting>    setting: one | three | default
      under ZK_BATCH_INV_ONE_LAUNCH_MAX as the parent sets it: per field, length and case of tests/batch_inverse_ref.py a digest of
      zk_upoly_batch_inverse's output with the count, the count, and a digest of the output of the same call without the count"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
from batch_inverse_ref import CHUNK, LENGTHS, cases  # noqa: E402
from field_corpus import worst_case_values  # noqa: E402

FIELD_IDS = ("bn254", "bls12_381", "bls12_377")
SWITCH = "ZK_BATCH_INV_ONE_LAUNCH_MAX"
# one: every length up to a chunk in one launch (the default, spelled out); three: the three launches at every length
SETTINGS = {"one": {SWITCH: str(CHUNK)}, "three": {SWITCH: "0"}, "default": {}}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def check(setting):
    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd import UnivariatePolynomial as UP

    assert os.environ.get(SWITCH) == SETTINGS[setting].get(SWITCH), os.environ.get(SWITCH)
    for fi, field in enumerate((zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR)):
        ctx = zk_amd.Context(field, 0)
        p = orc.modulus(field)
        for n_vars in (0, 1, 6, 8, 11, 12, 13):   # stale pool data in the size classes of the results and the scratch
            MLE.random(ctx, n_vars, 700 + n_vars).free()
        for n in LENGTHS:
            for name, vals, shift in cases(p, fi, n, worst_case_values):
                v = UP.new(ctx, orc.from_ints(field, vals))
                sh = orc.from_int(field, shift) if shift else None
                out, zeros = v.batch_inverse(shift=sh, count_zeros=True)
                quiet = v.batch_inverse(shift=sh)
                assert out.len() == n and quiet.len() == n
                print("DIGEST", FIELD_IDS[fi], f"n{n}_{name}", digest(out.coefficients()), zeros, digest(quiet.coefficients()))
        ctx.close()
    print(f"batch inverse {setting} ok")


if __name__ == "__main__":
    check(sys.argv[1])
