"""Structured inputs of the NTT family and the closed forms of their transforms (helper of tests/test_ntt_vectors_host.py,
tests/test_gpu_ntt_structured.py and tests/ntt_structured_check.py; no tests here).

The transforms keep their values lazily in [0, 2p) (zk_amd/csrc/ntt_kernels.cuh) and uniformly random inputs never make a butterfly
meet a + (p - a), a - a or s == 2p.  These inputs do: with n = 2^lg, w = orc.root_of_unity(field, n) and X[k] = sum_j x[j] w^(jk)

  zero          all 0                                        all 0
  constant      x[j] = c                                     X[0] = n c, every other output exactly 0
  impulse       x[j0] = c, j0 in {0, 1, n/2, n-1}            X[k] = c w^(j0 k)
  nyquist       x[j] = (-1)^j c                              n c at k = n/2, 0 elsewhere
  character     x[j] = c w^(-j k0), k0 in {1, n/2+1, n-1}    n c at k0, 0 elsewhere
  periodic      x[j + n/2] = x[j], first half random         every odd k exactly 0
  antiperiodic  x[j + n/2] = -x[j], first half random        every even k exactly 0 (every top-stage sum is p in the lazy domain)
  half_full     first half p - 1, second half 0              no closed form: the oracle only
  comb          p - 1 at even j, 0 at odd j                  X[0] = X[n/2] = (n/2)(p - 1), 0 elsewhere

c ranges over 1, p - 1 and one seeded random element.  Inputs are Montgomery limbs (orc.from_ints); every expectation is computed
from Python integers only, never through the oracle's transform."""
import random
from collections import namedtuple

import numpy as np

from oracle import binding as orc

FAMILIES = ("zero", "constant", "impulse", "nyquist", "character", "periodic", "antiperiodic", "half_full", "comb")
SPARSE = ("zero", "constant", "nyquist", "character", "comb")   # the whole spectrum is a few spikes

# x: the input; X: the whole expected transform or None; zeros: a slice of outputs that must be exactly 0 where only that is known;
# spikes: {k: canonical int} where the spectrum is nothing else
Case = namedtuple("Case", "name x X zeros spikes")


def omega(field, n, k0=1):
    """the canonical integer of w^k0, w the n-th root of unity the library and the oracle use"""
    return pow(orc.to_int(field, orc.root_of_unity(field, n)), k0, orc.modulus(field))


def values(field):
    p = orc.modulus(field)
    return [("1", 1), ("p-1", p - 1), ("r", random.Random(0xC0FFEE + field).randrange(2, p - 1))]


def half_random(field, lg):
    """the canonical integers of the random first half of the periodic and antiperiodic inputs"""
    return orc.to_ints(field, orc.fill_random(field, 0x57A7 + lg, max(1, (1 << lg) >> 1)))


def tiled(field, period, n):
    return np.ascontiguousarray(np.tile(orc.from_ints(field, period), (n // len(period), 1)))


def sparse(field, n, spikes):
    out = np.zeros((n, 4), dtype=np.uint64)
    for k, v in spikes.items():
        out[k] = orc.from_int(field, v)
    return out


def geometric(field, first, ratio, n):
    """first * ratio^j, j < n, as Montgomery limbs"""
    p = orc.modulus(field)
    vs, v = [0] * n, first % p
    for j in range(n):
        vs[j] = v
        v = v * ratio % p
    return orc.from_ints(field, vs)


def cases(field, lg, families=FAMILIES):
    """the Cases of the named families at n = 2^lg (lg >= 1), built one at a time"""
    p, n = orc.modulus(field), 1 << lg
    h = n // 2
    cs = values(field)
    for fam in families:
        if fam == "zero":
            yield Case("zero", np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64), None, {})
        elif fam == "constant":
            for cn, c in cs:
                sp = {0: n * c % p}
                yield Case(f"constant[{cn}]", tiled(field, [c], n), sparse(field, n, sp), None, sp)
        elif fam == "impulse":
            for j0 in sorted({0, 1, h, n - 1}):
                for cn, c in cs:
                    yield Case(f"impulse[{j0},{cn}]", sparse(field, n, {j0: c}), geometric(field, c, omega(field, n, j0), n), None, None)
        elif fam == "nyquist":
            for cn, c in cs:
                sp = {h: n * c % p}
                yield Case(f"nyquist[{cn}]", tiled(field, [c, p - c], n), sparse(field, n, sp), None, sp)
        elif fam == "character":
            for k0 in sorted({1 % n, (h + 1) % n, n - 1}):
                for cn, c in cs:
                    sp = {k0: n * c % p}
                    yield Case(f"character[{k0},{cn}]", geometric(field, c, omega(field, n, n - k0), n), sparse(field, n, sp), None, sp)
        elif fam == "periodic":
            a = half_random(field, lg)
            yield Case("periodic", orc.from_ints(field, a + a), None, slice(1, None, 2), None)
        elif fam == "antiperiodic":
            a = half_random(field, lg)
            yield Case("antiperiodic", orc.from_ints(field, a + [-v for v in a]), None, slice(0, None, 2), None)
        elif fam == "half_full":
            x = np.zeros((n, 4), dtype=np.uint64)
            x[:h] = orc.from_int(field, p - 1)
            yield Case("half_full", x, None, None, None)
        elif fam == "comb":
            sp = {0: h * (p - 1) % p, h: h * (p - 1) % p}
            yield Case("comb", tiled(field, [p - 1, 0], n), sparse(field, n, sp), None, sp)
        else:
            raise ValueError(fam)


def inverse_spikes(field, lg, spikes):
    """the inverse transform (1/n) sum_j x[j] w^(-jk) of an input whose forward transform is `spikes`: X[-k mod n] / n"""
    p, n = orc.modulus(field), 1 << lg
    n_inv = pow(n, -1, p)
    return {(-k) % n: v * n_inv % p for k, v in spikes.items()}
