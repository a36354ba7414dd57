"""The NTT family on structured inputs that hit exact zeros and p (tests/ntt_vectors.py).  Every transform keeps its values lazily
in [0, 2p) from the first load to the last store (zk_amd/csrc/ntt_kernels.cuh); random inputs never make a butterfly meet a + (p - a)
(zero carried as p through LDS, the inter-pass twiddles and the later passes), a - a, or s == 2p.  The device result is compared bit
for bit with orc.ntt_fast and, where one exists, with the closed form built from Python integers; above 2^17 with the closed forms
alone.  Plan shapes no other test runs: 2^14 (7,7) and 2^19 (7,6,6); 2^23 (8,8,7) otherwise runs only inside larger products."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc
from zk_amd import MultiLinearPolynomial as MLE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_vectors as nv  # noqa: E402
from ntt_structured_check import check_fft_cases  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
FIELD_IDS = ["bn254", "bls12_381", "bls12_377"]


@pytest.fixture
def make_ctx():
    """contexts that are closed when the test ends, passing or failing"""
    made = []

    def make(field):
        made.append(zk_amd.Context(field, 0))
        return made[-1]

    yield make
    for ctx in made:
        ctx.close()


@pytest.mark.parametrize("lg", [3, 7, 8, 11, 14, 16, 17])
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_fft_and_ifft_on_every_family(make_ctx, field, lg):
    """zk_fft_host / zk_ifft_host: the stage kernels below 2^8, two passes at 2^8 .. 2^16 (2^14 = (7,7)), three at 2^17; every
    family with every c at every position (tests/ntt_structured_check.py: check_fft_cases)"""
    assert check_fft_cases(make_ctx(field), field, lg, nv.cases(field, lg)) == 32


def _device_ntt(ctx, lg, x, inverse):
    src, dst = MLE.new(ctx, lg, x), MLE.alloc(ctx, lg)
    zk_amd.ntt(ctx, src, dst, inverse=inverse)
    out = dst.evaluation_slice()
    src.free()
    dst.free()
    return out


@pytest.mark.parametrize("family", ["constant", "nyquist", "character", "comb"])
@pytest.mark.parametrize("field", [zk_amd.BN254_FR, zk_amd.BLS12_381_FR], ids=["bn254", "bls12_381"])
def test_ntt_2p19_sparse_families_on_device_tables(make_ctx, field, family):
    """zk_ntt at 2^19, passes (7,6,6), both directions, against spectra built without a transform: forward x -> spikes, inverse
    x -> the spikes mirrored and divided by n, inverse spikes -> x; every c, and every k0 of the character with every c"""
    lg = 19
    n = 1 << lg
    ctx = make_ctx(field)
    done = 0
    for case in nv.cases(field, lg, (family,)):
        want = nv.sparse(field, n, case.spikes)
        assert np.array_equal(case.X, want)
        assert np.array_equal(_device_ntt(ctx, lg, case.x, False), want), ("forward", case.name)
        assert np.array_equal(_device_ntt(ctx, lg, case.x, True), nv.sparse(field, n, nv.inverse_spikes(field, lg, case.spikes))), (
            "inverse", case.name)
        assert np.array_equal(_device_ntt(ctx, lg, want, True), case.x), ("inverse of the spectrum", case.name)
        done += 1
    assert done == {"constant": 3, "nyquist": 3, "character": 9, "comb": 1}[family]


@pytest.mark.parametrize("field", [zk_amd.BN254_FR, zk_amd.BLS12_381_FR], ids=["bn254", "bls12_381"])
def test_ntt_2p19_antiperiodic_on_device_tables(make_ctx, field):
    """The antiperiodic input has no closed form for its odd outputs and 2^19 is past the size the oracle's transform is used at:
    every even output exactly 0 in both directions; 105 odd outputs per direction (the edges and 100 seeded ones) against the
    definition (orc.dft_point); and the inverse of the device's forward result returning x."""
    lg = 19
    n = 1 << lg
    ctx = make_ctx(field)
    (case,) = nv.cases(field, lg, ("antiperiodic",))
    rng = random.Random(0x0DD + field)
    odd = [1, 3, n // 2 - 1, n // 2 + 1, n - 1] + [2 * rng.randrange(n // 2) + 1 for _ in range(100)]
    fw = _device_ntt(ctx, lg, case.x, False)
    for inverse, got in ((False, fw), (True, _device_ntt(ctx, lg, case.x, True))):
        assert not got[case.zeros].any(), ("even outputs", inverse)
        for k in odd:
            assert np.array_equal(got[k], orc.dft_point(field, case.x, k, inverse=inverse)), ("odd output", k, inverse)
    assert np.array_equal(_device_ntt(ctx, lg, fw, True), case.x)


def test_ntt_2p23_constant_p_minus_1(make_ctx):
    """passes (8,8,7): X[0] = 2^23 (p - 1) mod p and the other 2^23 - 1 outputs hold no nonzero word"""
    field, lg = zk_amd.BN254_FR, 23
    p = orc.modulus(field)
    got = _device_ntt(make_ctx(field), lg, nv.tiled(field, [p - 1], 1 << lg), False)
    assert np.array_equal(got[0], orc.from_int(field, (p - 1) << lg))
    assert not got[1:].any()


@pytest.mark.parametrize("lg", [8, 13])
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_fft_internal_with_a_chosen_omega(make_ctx, field, lg):
    """zk_fft_internal_host with omega = w^5 (5 is odd: still primitive), tables built for that omega; the oracle's faithful recursion
    is the checker.  With v = w^5 the character x[j] = c v^(-j k0) transforms to n c at k0; the constant's spike stays at 0."""
    ctx = make_ctx(field)
    p, n = orc.modulus(field), 1 << lg
    v = nv.omega(field, n, 5)
    omega = orc.from_int(field, v)
    assert np.array_equal(omega, orc.pow_(field, orc.root_of_unity(field, n), 5))
    todo = list(nv.cases(field, lg, ("constant", "antiperiodic")))
    for k0 in (1, n // 2 + 1, n - 1):
        for cn, c in nv.values(field):
            sp = {k0: n * c % p}
            todo.append(nv.Case(f"character[{k0},{cn}]", nv.geometric(field, c, pow(v, n - k0, p), n), nv.sparse(field, n, sp), None, sp))
    assert len(todo) == 13
    for case in todo:
        want = np.zeros_like(case.x)
        orc._check(orc._lib.orc_fft_internal(field, orc._p(case.x), orc._c.c_uint64(n), orc._p(omega), orc._p(want)))
        got = zk_amd.fft_internal(ctx, case.x, omega)
        assert np.array_equal(got, want), (lg, case.name)
        if case.X is not None:
            assert np.array_equal(got, case.X), (lg, case.name)
        if case.zeros is not None:
            assert not got[case.zeros].any(), (lg, case.name)


def test_composed_interpass_twiddles_on_zero_as_p():
    """ZK_NTT_FULL_TABLE_MAX_LOG=0 (the switch tests/forced_paths_check.py forces): the passes compose their twiddles (ntt_twiddle:
    w_lo x w_hi by fe_mul29) instead of reading the full table, so a zero carried as p goes through that multiply.  One fresh child
    (tests/ntt_structured_check.py): antiperiodic and constant at 2^13 and 2^17 on BLS12-381."""
    env = dict(os.environ, ZK_NTT_FULL_TABLE_MAX_LOG="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ntt_structured_check.py")], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert "structured ntt ok: 8 cases (ZK_NTT_FULL_TABLE_MAX_LOG=0)" in r.stdout, r.stdout[-2000:]
