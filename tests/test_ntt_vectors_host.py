"""The closed forms of tests/ntt_vectors.py hold by the reference alone, before a GPU sees them: every family's expectation against
the oracle's iterative transform (orc.ntt_fast), against the faithful recursion (orc.fft, fft/src/lib.rs:21-46) up to 2^8, and the
oracle's inverse transform giving the input back."""
import os
import sys

import numpy as np
import pytest

import zk_amd
from oracle import binding as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_vectors as nv  # noqa: E402

FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]


@pytest.mark.parametrize("lg", [1, 3, 8, 12])
@pytest.mark.parametrize("field", FIELDS, ids=["bn254", "bls12_381", "bls12_377"])
def test_closed_forms_equal_the_oracle_transform(field, lg):
    n = 1 << lg
    seen = set()
    for case in nv.cases(field, lg):
        seen.add(case.name.split("[")[0])
        assert case.x.shape == (n, 4), case.name
        X = orc.ntt_fast(field, case.x)
        if case.X is not None:
            assert np.array_equal(X, case.X), case.name
        if case.zeros is not None:
            assert not X[case.zeros].any(), case.name
        if case.spikes is not None:
            assert np.array_equal(X, nv.sparse(field, n, case.spikes)), case.name
            ix = orc.ntt_fast(field, case.x, inverse=True)
            assert np.array_equal(ix, nv.sparse(field, n, nv.inverse_spikes(field, lg, case.spikes))), case.name
        assert (case.X is not None) or (case.zeros is not None) or case.name == "half_full"
        if lg <= 8:
            assert np.array_equal(orc.fft(field, case.x), X), case.name
        assert np.array_equal(orc.ntt_fast(field, X, inverse=True), case.x), case.name
    assert seen == set(nv.FAMILIES)


def test_the_inputs_are_what_the_table_says():
    """the structure the closed forms rest on, on canonical integers: x[j + n/2] = +-x[j], the character's ratio, every c used"""
    field, lg = zk_amd.BLS12_381_FR, 4
    p, n = orc.modulus(field), 16
    by_name = {c.name: orc.to_ints(field, c.x) for c in nv.cases(field, lg)}
    assert by_name["constant[p-1]"] == [p - 1] * n and by_name["nyquist[1]"] == [1, p - 1] * 8
    assert by_name["comb"] == [p - 1, 0] * 8 and by_name["half_full"] == [p - 1] * 8 + [0] * 8
    per, anti = by_name["periodic"], by_name["antiperiodic"]
    assert per[:8] == per[8:] == anti[:8] and all((a + b) % p == 0 for a, b in zip(anti[:8], anti[8:])) and len(set(per[:8])) == 8
    w = nv.omega(field, n)
    assert pow(w, 8, p) == p - 1
    ch = by_name["character[9,p-1]"]
    assert ch[0] == p - 1 and all(ch[j + 1] * pow(w, 9, p) % p == ch[j] for j in range(n - 1))
    assert by_name["impulse[15,r]"][:15] == [0] * 15 and by_name["impulse[15,r]"][15] == dict(nv.values(field))["r"]
