"""Tables built from RAW stored limbs (the Montgomery representation) at which the unreduced accumulators of the round and evaluate
kernels are tight, each with a closed form of what is asked of it.  Pure Python and numpy; test infrastructure only.

The kernels' bounds are stated over representations, not values: wide_mac / redc_wide take up to kMaxLazy = 32 products of
representations < p, dot29_mac / eval_mac sum products of 29-bit limbs of representations.  A table of the VALUE p - 1 stores
p - (R mod p), which is neither the largest representation nor one with large 29-bit limbs (tests/test_extreme_tables_host.py prints
and pins the numbers).  So, per field, with b = p.bit_length() and R = 2^256:

  M   = p - 1           the largest canonical representation: the largest wide top word
  O   = 2^(b-1) - 1     < p; split29 limbs 0..7 all ones, limb 8 as large as a canonical value allows; both 128-bit halves full of ones
  O1  = O - 1
  Z   = 0
  ONE = R mod p         the representation of the value 1

The value of a representation m is v(m) = m R^-1 mod p.  Families over n variables (every factor of a product is of the same family):

  const(m)       constant under every fold (lo == hi); round r has S_r(t) = 2^(n-1-r) prod v for every t; evaluate = prod v
  step(a, b)     the half of the index space that variable 0 pairs as "lo" holds a, the other b: round 0 sees hi - lo = b - a in every
                 pair, S_0(t) = 2^(n-1) prod (va + t (vb - va)); the fold at c leaves const(va + c (vb - va))
  stripe(a, b)   depends only on the variable folded LAST: every earlier round has hi - lo == 0 exactly in every pair (a leading
                 coefficient of exactly 0 next to maximal S(0), S(1)) and S_r(t) = 2^(n-2-r) (prod va + prod vb); the last round sees the
                 single pair (a, b)
  with_zero_factor   const(M) factors and one const(Z): every sum is exactly 0
  mixed          const(O) times seeded random factors: no closed form, the oracle is the check

Which half / stride is "lo" is taken from oracle/pyref.py's index_pair (pairing_index.rs), not assumed.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in (ROOT, os.path.join(ROOT, "tests")):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from field_corpus import K_MAX_LAZY, MODULI, R  # noqa: E402
from oracle import pyref  # noqa: E402

_W64 = (1 << 64) - 1


def raws(field):
    """the raw representations by name"""
    p = MODULI[field]
    o = (1 << (p.bit_length() - 1)) - 1
    return {"M": p - 1, "O": o, "O1": o - 1, "Z": 0, "ONE": R % p}


def value(field, m):
    """v(m) = m R^-1 mod p"""
    return m * pow(R, -1, MODULI[field]) % MODULI[field]


def rep(field, v):
    """the stored representation of the value v"""
    return v % MODULI[field] * R % MODULI[field]


def limbs(m):
    """raw representation -> (4,) uint64, least significant word first"""
    assert 0 <= m < R
    return np.array([(m >> (64 * i)) & _W64 for i in range(4)], dtype=np.uint64)


def elems(field, values):
    """canonical values -> (len, 4) uint64 stored limbs, through Python integers only"""
    return np.stack([limbs(rep(field, v)) for v in values]) if len(values) else np.zeros((0, 4), dtype=np.uint64)


def top_word(field, m, products=K_MAX_LAZY):
    """the 17th word of `products` accumulated squares of the representation m"""
    return (products * m * m) >> 512


def _pair_bit(n, last):
    """the index bit in which the pairs of partial_evaluate(var, ..) differ for var = 0 (last=False) or var = n - 1 (last=True), with
    lo = the index whose bit is 0: read off pyref.index_pair on a table of at most 6 variables, the first variable's bit counted from
    the top of the index and the last one's from the bottom"""
    m = min(n, 6)
    pairs = pyref.index_pair(m, m - 1 if last else 0)
    bits = {lo ^ hi for lo, hi in pairs}
    assert len(bits) == 1 and all(lo < hi for lo, hi in pairs)
    bit = bits.pop().bit_length() - 1
    return bit if last else (n - 1) - ((m - 1) - bit)


def const_table(m, n):
    return np.tile(limbs(m), (1 << n, 1))


def step_table(a, b, n):
    """lo half of variable 0's pairing holds a, hi half b"""
    if n == 0:
        return const_table(a, 0)
    sel = (np.arange(1 << n, dtype=np.uint64) >> np.uint64(_pair_bit(n, False))) & np.uint64(1)
    return np.where(sel[:, None] == 1, limbs(b)[None, :], limbs(a)[None, :])


def stripe_table(a, b, n):
    """lo side of the LAST variable's pairing holds a, hi side b"""
    if n == 0:
        return const_table(a, 0)
    sel = (np.arange(1 << n, dtype=np.uint64) >> np.uint64(_pair_bit(n, True))) & np.uint64(1)
    return np.where(sel[:, None] == 1, limbs(b)[None, :], limbs(a)[None, :])


class Closed:
    """closed form of a product of same-family factors: kind in {"const", "step", "stripe"}, params = [(va, vb)] canonical values per
    factor (const: va == vb)"""

    def __init__(self, field, n, kind, params):
        self.field, self.n, self.kind, self.params = field, n, kind, [(a % MODULI[field], b % MODULI[field]) for a, b in params]
        self.p = MODULI[field]

    def _prod(self, vals):
        out = 1
        for v in vals:
            out = out * v % self.p
        return out

    def round_sum(self, t):
        """S(t) of the first round: sum over the pairs of prod_f (lo + t (hi - lo))"""
        p, n = self.p, self.n
        assert n >= 1
        if self.kind == "const":
            return (1 << (n - 1)) * self._prod(a for a, _ in self.params) % p
        if self.kind == "step" or n == 1:
            return (1 << (n - 1)) * self._prod(a + t * (b - a) for a, b in self.params) % p
        return (1 << (n - 2)) * (self._prod(a for a, _ in self.params) + self._prod(b for _, b in self.params)) % p

    def round_sums(self, D):
        return [self.round_sum(t) for t in range(D + 1)]

    def fold(self, c):
        """the product after partial_evaluate(0, [c])"""
        if self.kind == "const" or (self.kind == "stripe" and self.n > 1):
            return Closed(self.field, self.n - 1, self.kind, self.params)
        w = [(a + c * (b - a)) % self.p for a, b in self.params]
        return Closed(self.field, self.n - 1, "const", [(x, x) for x in w])

    def true_sum(self):
        return (self.round_sum(0) + self.round_sum(1)) % self.p if self.n else self._prod(a for a, _ in self.params)

    def prove(self, D, claimed):
        """prove_partial (prover.rs:33-73): -> (round polys [n][D+1], challenges [n]) as canonical values; the transcript is pyref's"""
        tr = pyref.Transcript()
        tr.append((claimed % self.p).to_bytes(32, "big"))
        cur, rps, chs = self, [], []
        for _ in range(self.n):
            rp = cur.round_sums(D)
            tr.append(b"".join(v.to_bytes(32, "big") for v in rp))
            c = tr.sample_field_element(self.field)
            cur = cur.fold(c)
            rps.append(rp)
            chs.append(c)
        return rps, chs

    def round_polys(self, D, challenges):
        """the round polynomials of a proof whose challenges (canonical values) are given"""
        cur, rps = self, []
        for c in challenges:
            rps.append(cur.round_sums(D))
            cur = cur.fold(c % self.p)
        return rps

    def evaluate(self, point):
        cur = self
        for c in point:
            cur = cur.fold(c % self.p)
        assert cur.n == 0
        return cur._prod(a for a, _ in cur.params)

    def factor(self, f):
        return Closed(self.field, self.n, self.kind, [self.params[f]])


FAMILIES = ("const(M)", "const(O)", "step(Z,O)", "step(O,Z)", "step(M,Z)", "stripe(M,Z)", "stripe(O,O1)", "with_zero_factor", "mixed")
_TWO_RAW = {"step(Z,O)": ("step", "Z", "O"), "step(O,Z)": ("step", "O", "Z"), "step(M,Z)": ("step", "M", "Z"),
            "stripe(M,Z)": ("stripe", "M", "Z"), "stripe(O,O1)": ("stripe", "O", "O1"), "stripe(O,Z)": ("stripe", "O", "Z"),
            "const(M)": ("const", "M", "M"), "const(O)": ("const", "O", "O"), "const(Z)": ("const", "Z", "Z"),
            "const(ONE)": ("const", "ONE", "ONE")}
_BUILD = {"const": lambda a, b, n: const_table(a, n), "step": step_table, "stripe": stripe_table}


def table(field, name, n):
    """one table of a named single-factor family -> (2^n, 4) uint64"""
    kind, a, b = _TWO_RAW[name]
    r = raws(field)
    return _BUILD[kind](r[a], r[b], n)


def family(field, name, n, k, fill_random=None, seed=0):
    """k factor tables of the family and its closed form (None for "mixed") -> ([tables], Closed or None).  Equal factors are the SAME
    array object, so a caller may upload each distinct table once.  fill_random(field, seed, count) supplies the random factors of
    "mixed" (the oracle's generator)."""
    r = raws(field)
    if name == "with_zero_factor":
        m, z = const_table(r["M"], n), const_table(r["Z"], n)
        tabs = [m] * (k - 1) + [z]
        vm = value(field, r["M"])
        return tabs, Closed(field, n, "const", [(vm, vm)] * (k - 1) + [(0, 0)])
    if name == "mixed":
        o = const_table(r["O"], n)
        return [o] + [fill_random(field, seed + f, 1 << n) for f in range(1, k)], None
    kind, a, b = _TWO_RAW[name]
    t = _BUILD[kind](r[a], r[b], n)
    va, vb = value(field, r[a]), value(field, r[b])
    return [t] * k, Closed(field, n, kind, [(va, vb)] * k)
