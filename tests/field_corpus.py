"""Corpus and big-int model for the field-primitive harness (tests/cpp/test_field_device.hip).

Pure Python, deterministic (seeded).  For each field it builds, per primitive, the operands the harness runs and the output
limbs it must produce -- the expected values are Python integers, nothing else.  The operands are chosen by LIMB PATTERN, not
only by value: every 32-bit word all ones / all zeros, every 29-bit limb all ones / all zeros at the cuts of split29 (bit 29 i)
and of split29_shl5 (bit 29 i - 5), powers of two and their neighbours, values a few units from p, 2p and 2^256 where the
primitive's documented domain admits them.  Two-operand primitives get the FULL cross product of the structured values (the
harness forms it: the case file carries the two lists), plus seeded random pairs, plus pairs filtered by the model so that each
side of every final conditional step has cases and its exact boundary is present (tests/test_field_corpus_host.py counts them).

Domains (each next to the line that promises it):
  fe_add / fe_sub / fe_neg / fe_mul / fe_sqr / redc      a, b < p        field.cuh "always fully reduced (< p)"
  wide_mac x N + redc_wide                               N <= kMaxLazy = 32 products of values < p   field.cuh redc_wide comment
  fe_mul29 / fe_mul29_t<true>                            a ANY 256-bit value, c < p   field.cuh mul29_core: "in [0, 2p) for ANY 256-bit a"
  fe_mul_tt                                              a, b < p (a * 2^5 < 2^260)   field.cuh fe_mul_tt comment
  fe_dot2_29                                             a, a2 < p, c, c2 < p         field.cuh mul29_core TWO comment
  fe_add2 / fe_sub2 / fe_canon2                          a, b < 2p       ntt_kernels.cuh "Values stay in [0, 2p)"
  fe_reduce_u256                                         any 256-bit x   field.cuh fe_reduce_u256 comment
  fe_from_canonical / fe_to_canonical                    x < p           field.cuh conversions
  fe_from_u32                                            any u32
"""
import random
import struct

import numpy as np

# ark-bn254 / ark-bls12-381 / ark-bls12-377 Fr (the moduli of zk_amd/csrc/host_field.hpp)
MODULI = (
    0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
    0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
    0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001,
)
FIELD_NAMES = ("bn254", "bls12-381", "bls12-377")
R = 1 << 256
W = 1 << 261          # the 29-bit core divides by 2^261
K_MAX_LAZY = 32       # field.cuh kMaxLazy
MAGIC = 0x46454431

# primitive ids of the harness (enum Op)
(OP_ADD, OP_SUB, OP_NEG, OP_MUL, OP_SQR, OP_MULWIDE_REDC, OP_WIDE, OP_MUL29, OP_MUL29_LAZY, OP_MUL_TT, OP_DOT2, OP_ADD2, OP_SUB2,
 OP_CANON2, OP_REDUCE_U256, OP_FROM_CANONICAL, OP_TO_CANONICAL, OP_FROM_U32, OP_PREPARE) = range(19)
OP_NAMES = ("fe_add", "fe_sub", "fe_neg", "fe_mul", "fe_sqr", "mul_wide+redc", "wide_mac+redc_wide", "fe_mul29", "fe_mul29_t<true>",
            "fe_mul_tt", "fe_dot2_29", "fe_add2", "fe_sub2", "fe_canon2", "fe_reduce_u256", "fe_from_canonical", "fe_to_canonical",
            "fe_from_u32", "mul29_prepare")
DEVICE_ONLY = (OP_ADD2, OP_SUB2, OP_CANON2)   # ntt_kernels.cuh helpers: not in the host build of the harness
N_RANDOM = 4096       # seeded random cases added to every section (the part to shrink if the suite time matters, never the structured part)
N_FILTER = 320        # cases collected per side of a branch by model-filtered search (the host test asserts >= 256 per side)


class FieldModel:
    """the constants of one field as Python integers"""

    def __init__(self, field):
        self.field = field
        self.p = p = MODULI[field]
        self.rinv = pow(R, -1, p)
        self.r1 = R % p
        self.r2 = R * R % p
        self.ninv_r = (-pow(p, -1, R)) % R      # -p^-1 mod 2^256
        self.ninv_w = (-pow(p, -1, W)) % W      # -p^-1 mod 2^261
        self.top_max = K_MAX_LAZY * p * p >> 512

    # ---- pre-subtraction values of the multipliers (what the final conditional step decides on) ----
    def redc_pre(self, t):
        """(t + m p) / 2^256 with m = -t p^-1 mod 2^256: the value redc holds before its conditional subtraction"""
        m = (t * self.ninv_r) % R
        return (t + m * self.p) >> 256

    def core_pre(self, a, c, a2=0, c2=0):
        """the exact integer mul29_core holds before its conditional subtraction: (a c' + a2 c2' + m p) / 2^261, c' = 32 c mod p"""
        p = self.p
        t = a * (32 * c % p) + a2 * (32 * c2 % p)
        m = (t * self.ninv_w) % W
        return (t + m * p) >> 261


def split29(x):
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [x >> 232]


# ---- expected outputs: (value, number of 32-bit words) lists per case, and the side of the final conditional step ----------------
def model(fm, op, cols, param=0):
    """-> (outs, taken): outs = list of per-case tuples of (integer, words) outputs; taken = list of bool (or None: no final
    conditional step to count) saying whether the primitive's last conditional step takes its subtract / add-back side"""
    p, rinv = fm.p, fm.rinv
    if op == OP_ADD:
        a, b = cols
        return [(((x + y) % p, 8),) for x, y in zip(a, b)], [x + y >= p for x, y in zip(a, b)]
    if op == OP_SUB:
        a, b = cols
        return [(((x - y) % p, 8),) for x, y in zip(a, b)], [x < y for x, y in zip(a, b)]
    if op == OP_NEG:
        return [((-x % p, 8),) for x in cols[0]], [x != 0 for x in cols[0]]
    if op in (OP_MUL, OP_MUL_TT):
        a, b = cols
        outs = [((x * y * rinv % p, 8),) for x, y in zip(a, b)]
        if op == OP_MUL:
            return outs, [fm.redc_pre(x * y) >= p for x, y in zip(a, b)]
        return outs, [_tt_pre(fm, x, y) >= p for x, y in zip(a, b)]
    if op == OP_SQR:
        return [((x * x * rinv % p, 8),) for x in cols[0]], [fm.redc_pre(x * x) >= p for x in cols[0]]
    if op == OP_MULWIDE_REDC:
        a, b = cols
        return [((x * y, 16), (x * y * rinv % p, 8)) for x, y in zip(a, b)], [fm.redc_pre(x * y) >= p for x, y in zip(a, b)]
    if op == OP_WIDE:
        outs = []
        for row in zip(*cols):
            w = sum(row[2 * i] * row[2 * i + 1] for i in range(param))
            outs.append(((w, 17), (w * rinv % p, 8)))
        return outs, None
    if op == OP_MUL29:
        a, c = cols
        return [((x * y * rinv % p, 8),) for x, y in zip(a, c)], [fm.core_pre(x, y) >= p for x, y in zip(a, c)]
    if op == OP_MUL29_LAZY:
        a, c = cols
        return [((fm.core_pre(x, y), 8),) for x, y in zip(a, c)], None
    if op == OP_DOT2:
        a, c, a2, c2 = cols
        return ([(((x * y + x2 * y2) * rinv % p, 8),) for x, y, x2, y2 in zip(a, c, a2, c2)],
                [fm.core_pre(x, y, x2, y2) >= p for x, y, x2, y2 in zip(a, c, a2, c2)])
    if op == OP_ADD2:
        a, b = cols
        return [(((x + y) % (2 * p), 8),) for x, y in zip(a, b)], [x + y >= 2 * p for x, y in zip(a, b)]
    if op == OP_SUB2:
        a, b = cols
        return [(((x - y) % (2 * p), 8),) for x, y in zip(a, b)], [x < y for x, y in zip(a, b)]
    if op == OP_CANON2:
        return [((x % p, 8),) for x in cols[0]], [x >= p for x in cols[0]]
    if op == OP_REDUCE_U256:
        return [((x % p, 8),) for x in cols[0]], None
    if op in (OP_FROM_CANONICAL, OP_FROM_U32):
        return [((x * R % p, 8),) for x in cols[0]], [fm.redc_pre(x * fm.r2) >= p for x in cols[0]]
    if op == OP_TO_CANONICAL:
        return [((x * rinv % p, 8),) for x in cols[0]], [fm.redc_pre(x) >= p for x in cols[0]]
    if op == OP_PREPARE:
        return [tuple((l, 1) for l in split29(32 * x % p)) for x in cols[0]], None
    raise ValueError(op)


def _tt_pre(fm, a, b):
    """fe_mul_tt's pre-subtraction value: ((a 2^5) b + m p) / 2^261 (the left operand is SPLIT five bits lower, b is not prepared)"""
    t = (a << 5) * b
    m = (t * fm.ninv_w) % W
    return (t + m * fm.p) >> 261


# ---- structured values ---------------------------------------------------------------------------------------------------
def _patterns(rng):
    """256-bit values with one 32-bit word, or one 29-bit limb at the split29 / split29_shl5 cuts, all ones and all zeros over
    random other bits"""
    out = []
    spans = [(32 * i, 32) for i in range(8)]
    spans += [(29 * i, 29 if i < 8 else 24) for i in range(9)]                        # split29: limb i starts at bit 29 i
    spans += [(0, 24)] + [(29 * i - 5, 29) for i in range(1, 9)]                      # split29_shl5: limb i starts at bit 29 i - 5
    for lo, width in spans:
        mask = ((1 << width) - 1) << lo
        for _ in range(2):
            v = rng.getrandbits(256)
            out.append(v | mask)
            out.append(v & ~mask)
    # every limb of a cut all ones / alternating all ones and all zeros
    for start, first in ((0, 29), (0, 24)):
        v, bit, on = 0, 0, True
        width = first
        while bit < 256:
            if on:
                v |= ((1 << width) - 1) << bit
            bit, width, on = bit + width, 29, not on
        v &= R - 1
        out += [v, v ^ (R - 1)]
    return out


def _clip(v, bound):
    """the largest low-bit truncation of v below bound (keeps the low-order pattern, drops top bits until the value is in range)"""
    k = 256
    while v >= bound:
        k -= 1
        v &= (1 << k) - 1
    return v


def _dedupe(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def structured_values(fm, domain, rng):
    """domain: 'canon' (< p), 'lazy' (< 2p) or 'any' (< 2^256)"""
    p = fm.p
    bound = {"canon": p, "lazy": 2 * p, "any": R}[domain]
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, fm.r1, fm.r2, p - fm.r1]
    for k in range(256):
        vals += [v for v in (1 << k, (1 << k) - 1, p - (1 << k)) if 0 <= v < bound]
    if domain != "canon":
        vals += [v for v in (p, p + 1, 2 * p - 1, 2 * p - 2, 2 * p - 3, p + fm.r1, 2 * p - fm.r1) if v < bound]
        for k in range(256):
            vals += [v for v in (2 * p - (1 << k), p + (1 << k)) if p <= v < bound]
    if domain == "any":
        vals += [2 * p, 2 * p + 1, R - 1, R - 2]
        vals += [R - (1 << k) for k in range(256)]
        vals += [j * p + d for j in range(3, (R - 1) // p + 1) for d in (-1, 0, 1) if j * p + d < R]   # around every multiple of p below 2^256
    vals += [_clip(v, bound) for v in _patterns(rng)]
    return _dedupe(vals)


def worst_case_values(p, field_index, n):
    """n canonical ints whose Montgomery limbs are the structured worst cases above (p - 1, powers of two and their neighbours,
    all-ones / all-zeros words and 29-bit limbs), for tests that feed whole tables of them to a kernel"""
    fm = FieldModel(MODULI.index(p))
    vals = structured_values(fm, "canon", random.Random(0xD1F + field_index))
    random.Random(field_index).shuffle(vals)
    return [v * fm.rinv % p for v in vals[:n]]


def random_values(rng, bound, n):
    bits = bound.bit_length()
    out = []
    while len(out) < n:
        v = rng.getrandbits(bits)
        if v < bound:
            out.append(v)
    return out


class Section:
    """cases of one primitive: either explicit rows (cols: one list of integers per operand) or the cross product of two lists"""

    def __init__(self, op, cols=None, cross=None, param=0, words=8, label=""):
        self.op, self.param, self.words, self.label = op, param, words, label
        self.cross = cross
        self._cols = cols

    @property
    def n(self):
        return len(self.cross[0]) * len(self.cross[1]) if self.cross else len(self._cols[0])

    def cols(self):
        """operand columns, the cross product written out in the harness's order (case i = (A[i // nB], B[i % nB]))"""
        if not self.cross:
            return self._cols
        a, b = self.cross
        return [[x for x in a for _ in b], list(b) * len(a)]

    def case(self, i):
        if self.cross:
            a, b = self.cross
            return (a[i // len(b)], b[i % len(b)])
        return tuple(c[i] for c in self._cols)


def _limbs(vals, words=8):
    """list of integers -> (n, words) uint32 array, little-endian limbs"""
    buf = b"".join(v.to_bytes(4 * words, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u4").reshape(len(vals), words)


def _search(rng, draw, pred, n, limit=1_000_000):
    """n cases from draw() that satisfy pred (the model decides: nothing is assumed about how often it holds)"""
    out = []
    for _ in range(limit):
        c = draw()
        if pred(*c):
            out.append(c)
            if len(out) == n:
                return out
    raise RuntimeError(f"only {len(out)} of {n} filtered cases found")


def _columns(rows):
    return [list(c) for c in zip(*rows)]


def build_sections(field, n_random=N_RANDOM):
    """every section of one field's corpus, in file order"""
    fm = FieldModel(field)
    p = fm.p
    rng = random.Random(0xF1E1D000 + field)
    canon = structured_values(fm, "canon", rng)
    lazy = structured_values(fm, "lazy", rng)
    anyv = structured_values(fm, "any", rng)
    rc = lambda n: random_values(rng, p, n)          # noqa: E731
    secs = []

    def pairs_random(op, da, db, label="random"):
        bounds = {"canon": p, "lazy": 2 * p, "any": R}
        secs.append(Section(op, cols=[random_values(rng, bounds[da], n_random), random_values(rng, bounds[db], n_random)], label=label))

    big = lambda: p - 1 - rng.getrandbits(200)       # noqa: E731  (values just below p: where the multipliers' final subtraction is likeliest)

    # -- fe_add / fe_sub / fe_neg: a, b < p ------------------------------------------------------------------------------
    for op in (OP_ADD, OP_SUB):
        secs.append(Section(op, cross=(canon, canon), label="structured x structured"))
        pairs_random(op, "canon", "canon")
    xs = rc(N_FILTER)
    #   the exact boundary of fe_add's `s >= p`: a + b = p - 1, p, p + 1 (results p - 1, 0, 1), over random and structured a
    for d in (-1, 0, 1):
        rows = [(x, p + d - x) for x in xs + canon if 0 <= p + d - x < p]
        secs.append(Section(OP_ADD, cols=_columns(rows), label=f"a + b = p {d:+d}"))
    #   fe_sub's borrow boundary: a - b = -1, 0, 1 (results p - 1, 0, 1)
    for d in (-1, 0, 1):
        rows = [(x, x - d) for x in xs + canon if 0 <= x - d < p]
        secs.append(Section(OP_SUB, cols=_columns(rows), label=f"a - b = {d:+d}"))
    secs.append(Section(OP_NEG, cols=[canon + rc(n_random)], label="structured + random"))

    # -- fe_mul / fe_sqr / mul_wide + redc / fe_mul_tt: a, b < p ---------------------------------------------------------
    for op in (OP_MUL, OP_MULWIDE_REDC, OP_MUL_TT):
        secs.append(Section(op, cross=(canon, canon), label="structured x structured"))
        pairs_random(op, "canon", "canon")
    secs.append(Section(OP_SQR, cols=[canon + rc(n_random)], label="structured + random"))
    #   results 0, 1 and p - 1 on BOTH sides of the final subtraction where the arithmetic allows it (pre-subtraction value
    #   1 / p + 1 and p - 1; a pre-subtraction value of exactly p needs p | a b, impossible for 0 < a, b < p): b = +-R a^-1
    for op, pre in ((OP_MUL, lambda a, b: fm.redc_pre(a * b)), (OP_MULWIDE_REDC, lambda a, b: fm.redc_pre(a * b)),
                    (OP_MUL_TT, lambda a, b: _tt_pre(fm, a, b))):
        def with_result(res):
            a = big()
            return (a, res * R * pow(a, -1, p) % p)
        rows = _search(rng, lambda: with_result(1), lambda a, b: pre(a, b) == p + 1, 4)
        rows += _search(rng, lambda: with_result(p - 1), lambda a, b: pre(a, b) == p - 1, 4)
        rows += [(1, fm.r1), (fm.r1, 1), (1, (p - 1) * R % p), ((p - 1) * R % p, 1)]   # results 1 and p - 1 from a small operand
        rows += [(0, x) for x in xs[:4]] + [(x, 0) for x in xs[:4]]
        secs.append(Section(op, cols=_columns(rows), label="pre-subtraction value p + 1, p - 1; results 0, 1, p - 1"))
        #   the taken side of the final subtraction, counted by the model (rare for fe_mul_tt: about a b / (2^256 p))
        rows = _search(rng, lambda: (big(), big()), lambda a, b: pre(a, b) >= p, N_FILTER)
        secs.append(Section(op, cols=_columns(rows), label="final subtraction taken (filtered)"))

    # -- wide_mac x N + redc_wide: N products of values < p -----------------------------------------------------------------
    pool = canon + rc(256)
    for N in (1, 2, 31, K_MAX_LAZY):
        n_rows = 2048 if N <= 2 else 512
        rows = [[p - 1] * (2 * N), [0] * (2 * N), [p - 1, 1] * N, [p - 1, p - 2] * N]   # all p - 1: the top limb reaches its maximum at N = 32
        rows += [[p - 1 - rng.getrandbits(8) for _ in range(2 * N)] for _ in range(64)]
        rows += [[rng.choice(pool) for _ in range(2 * N)] for _ in range(n_rows // 2)]
        rows += [rc(2 * N) for _ in range(n_rows // 2)]
        secs.append(Section(OP_WIDE, cols=_columns(rows), param=N, label=f"N = {N}"))

    # -- fe_mul29 / fe_mul29_t<true>: a ANY 256-bit value, c < p -----------------------------------------------------------
    for op in (OP_MUL29, OP_MUL29_LAZY):
        secs.append(Section(op, cross=(anyv, canon), label="any-256-bit structured x structured"))
        pairs_random(op, "any", "canon")
        #   a = p is the lazy-domain zero: the pre-subtraction value is exactly p for every c != 0
        secs.append(Section(op, cols=[[p] * (N_FILTER + len(canon)), rc(N_FILTER) + canon], label="a = p (pre-subtraction value == p)"))
        #   pre-subtraction value p - 1, p + 1 and 1: result p - 1 / 1, c = +-R a^-1, a anywhere in 256 bits
        def with_result29(res, canonical):
            a = big() if canonical else R - 1 - rng.getrandbits(250)
            if a % p == 0:
                a -= 1
            return (a, res * R * pow(a, -1, p) % p)
        rows = []
        for canonical in (False, True):
            rows += _search(rng, lambda: with_result29(1, canonical), lambda a, c: fm.core_pre(a, c) == p + 1, 4)
            rows += _search(rng, lambda: with_result29(p - 1, canonical), lambda a, c: fm.core_pre(a, c) == p - 1, 4)
        rows += [(1, fm.r1), (fm.r1, 1), (1, (p - 1) * R % p), (0, fm.r1), (fm.r1, 0), (p, 0), (2 * p, fm.r1)]
        secs.append(Section(op, cols=_columns(rows), label="pre-subtraction value p + 1, p - 1; results 0, 1, p - 1"))
        #   the taken side with CANONICAL a (what folds and canonical transforms feed): rare, so filtered by the model
        rows = _search(rng, lambda: (big(), rng.randrange(p)), lambda a, c: fm.core_pre(a, c) >= p, N_FILTER)
        secs.append(Section(op, cols=_columns(rows), label="canonical a, final subtraction taken (filtered)"))
        #   and with a in [p, 2p) and in [2p, 2^256)
        rows = _search(rng, lambda: (rng.randrange(p, 2 * p), rng.randrange(p)), lambda a, c: fm.core_pre(a, c) >= p, N_FILTER)
        rows += _search(rng, lambda: (rng.randrange(2 * p, R), rng.randrange(p)), lambda a, c: fm.core_pre(a, c) >= p, N_FILTER)
        secs.append(Section(op, cols=_columns(rows), label="lazy and any-256-bit a, final subtraction taken (filtered)"))
    secs.append(Section(OP_PREPARE, cols=[canon + rc(n_random)], label="structured + random"))

    # -- fe_dot2_29: a, a2 < p; c, c2 < p ------------------------------------------------------------------------------------
    rows = [[rng.choice(canon) for _ in range(4)] for _ in range(16 * n_random)]
    rows += [rc(4) for _ in range(n_random)]
    rows += [[p - 1] * 4, [0] * 4, [p - 1, 1, p - 1, 1], [1, p - 1, 1, p - 1], [p - 1, p - 1, 0, 0], [0, 0, p - 1, p - 1]]
    secs.append(Section(OP_DOT2, cols=_columns(rows), label="structured and random quadruples"))
    rows = _search(rng, lambda: (big(), big(), big(), big()), lambda a, c, a2, c2: fm.core_pre(a, c, a2, c2) >= p, N_FILTER)
    #   results 0 (a c = -a2 c2), 1 and p - 1
    for res in (0, 1, p - 1):
        for _ in range(8):
            a, c, a2 = big(), rng.randrange(1, p), big()
            rows.append((a, c, a2, (res * R - a * c) * pow(a2, -1, p) % p))
    secs.append(Section(OP_DOT2, cols=_columns(rows), label="final subtraction taken (filtered); results 0, 1, p - 1"))

    # -- fe_add2 / fe_sub2 / fe_canon2: values in [0, 2p) -------------------------------------------------------------------------
    for op in (OP_ADD2, OP_SUB2):
        secs.append(Section(op, cross=(lazy, lazy), label="lazy structured x structured"))
        pairs_random(op, "lazy", "lazy")
    xs2 = random_values(rng, 2 * p, N_FILTER)
    for d in (-1, 0, 1):
        rows = [(x, 2 * p + d - x) for x in xs2 + lazy if 0 <= 2 * p + d - x < 2 * p]
        secs.append(Section(OP_ADD2, cols=_columns(rows), label=f"a + b = 2p {d:+d}"))
        rows = [(x, x - d) for x in xs2 + lazy if 0 <= x - d < 2 * p]
        secs.append(Section(OP_SUB2, cols=_columns(rows), label=f"a - b = {d:+d}"))
    if 4 * p > R:   # BLS12-381 only: a + b can carry out of 2^256
        rows = []
        for d in (-2, -1, 0, 1, 2):
            lo = R + d - (2 * p - 1)
            rows += [(x, R + d - x) for x in [lo, 2 * p - 1, p, R + d - p] + [rng.randrange(lo, 2 * p) for _ in range(N_FILTER)]]
        rows += [(2 * p - 1, 2 * p - 1), (2 * p - 1, 2 * p - 2)]
        assert all(0 <= a < 2 * p and 0 <= b < 2 * p for a, b in rows)
        secs.append(Section(OP_ADD2, cols=_columns(rows), label="a + b within 2 of 2^256 (carry out)"))
    secs.append(Section(OP_CANON2, cols=[lazy + random_values(rng, 2 * p, n_random)], label="structured + random"))

    # -- fe_reduce_u256: any 256-bit x; conversions ----------------------------------------------------------------------------------
    secs.append(Section(OP_REDUCE_U256, cols=[anyv + random_values(rng, R, n_random)], label="structured + random"))
    for op in (OP_FROM_CANONICAL, OP_TO_CANONICAL):
        secs.append(Section(op, cols=[canon + rc(n_random)], label="structured + random"))
    #   (fe_to_canonical reduces t = a < p: (a + m p) / 2^256 < p always, its final subtraction is never taken)
    rows = _search(rng, lambda: (rng.randrange(p),), lambda x: fm.redc_pre(x * fm.r2) >= p, N_FILTER)
    secs.append(Section(OP_FROM_CANONICAL, cols=_columns(rows), label="final subtraction taken (filtered)"))
    u32 = _dedupe([0, 1, 2, 0xFFFFFFFF, 0xFFFFFFFE] + [1 << k for k in range(32)] + [(1 << k) - 1 for k in range(32)]
                  + [rng.getrandbits(32) for _ in range(n_random)])
    secs.append(Section(OP_FROM_U32, cols=[u32], words=1, label="structured + random"))
    return fm, secs


# ---- the case file and the expected output ---------------------------------------------------------------------------------
def case_file_bytes(field, secs):
    parts = [struct.pack("<3I", MAGIC, field, len(secs))]
    for s in secs:
        if s.cross:
            a, b = s.cross
            parts.append(struct.pack("<5I", s.op, s.param, 1, len(a), len(b)))
            parts += [_limbs(a).tobytes(), _limbs(b).tobytes()]
        else:
            cols = s.cols()
            parts.append(struct.pack("<5I", s.op, s.param, 0, len(cols[0]), 0))
            parts.append(np.concatenate([_limbs(c, s.words) for c in cols], axis=1).tobytes())
    return b"".join(parts)


def expected_words(fm, s):
    """(n, out_words) uint32 array the harness must write for section s, and the per-case branch sides (or None)"""
    outs, taken = model(fm, s.op, s.cols(), s.param)
    n_out = len(outs[0])
    arrs = [_limbs([o[j][0] for o in outs], outs[0][j][1]) for j in range(n_out)]
    return np.concatenate(arrs, axis=1), taken


def out_words(op):
    return {OP_MULWIDE_REDC: 24, OP_WIDE: 25, OP_PREPARE: 9}.get(op, 8)


def out_offsets(secs):
    """word offset of every section's output in the harness's output file, and the total"""
    offs, pos = [], 0
    for s in secs:
        offs.append(pos)
        pos += s.n * out_words(s.op)
    return offs, pos


# ---- checking a harness output against the model, one section per task (worker processes: the model is the slow side) ----------
_BUILT = {}


def built(field):
    if field not in _BUILT:
        _BUILT[field] = build_sections(field)
    return _BUILT[field]


def check_section(task):
    """task = (field, section index, {build name: output file}, ops left out of those files) -> dict with the section's size, the
    number of cases on the taken side of its final conditional step (None where there is none), its boundary facts, and per build
    the number of mismatching limbs and the first failing case"""
    field, idx, outputs, skip_ops = task
    fm, secs = built(field)
    s = secs[idx]
    want, taken = expected_words(fm, s)
    if s.op in skip_ops:
        outputs = {}
    else:
        kept = [t for t in secs if t.op not in skip_ops]
        offs, total = out_offsets(kept)
        idx = kept.index(s)
    res = {"field": field, "op": s.op, "label": s.label, "n": s.n, "taken": None if taken is None else sum(taken),
           "facts": _facts(fm, s, want), "builds": {}}
    for name, path in outputs.items():
        got = np.memmap(path, dtype="<u4", mode="r")
        if got.size != total:
            res["builds"][name] = {"bad_limbs": -1, "first": None, "note": f"output has {got.size} words, expected {total}"}
            continue
        got = got[offs[idx]:offs[idx] + want.size].reshape(want.shape)
        diff = got != want
        bad = int(diff.sum())
        first = None
        if bad:
            i = int(np.argmax(diff.any(axis=1)))
            first = {"case": i, "operands": [hex(v) for v in s.case(i)], "got": [hex(int(w)) for w in got[i]],
                     "want": [hex(int(w)) for w in want[i]]}
        res["builds"][name] = {"bad_limbs": bad, "first": first}
    return res


def _facts(fm, s, want):
    """boundary facts of a section that the corpus conditions ask for (tests/test_field_corpus_host.py)"""
    p = fm.p
    facts = set()
    cols = None
    if s.op in (OP_MUL29, OP_MUL29_LAZY, OP_DOT2, OP_MUL, OP_MULWIDE_REDC, OP_MUL_TT, OP_ADD, OP_ADD2, OP_CANON2) and s.n <= 20000:
        cols = s.cols()
        if s.op in (OP_MUL29, OP_MUL29_LAZY):
            pres = [fm.core_pre(a, c) for a, c in zip(*cols)]
        elif s.op == OP_DOT2:
            pres = [fm.core_pre(*r) for r in zip(*cols)]
        elif s.op == OP_MUL_TT:
            pres = [_tt_pre(fm, a, b) for a, b in zip(*cols)]
        elif s.op in (OP_MUL, OP_MULWIDE_REDC):
            pres = [fm.redc_pre(a * b) for a, b in zip(*cols)]
        elif s.op == OP_CANON2:
            pres = list(cols[0])
        else:
            pres = [a + b for a, b in zip(*cols)]
        edge = 2 * p if s.op == OP_ADD2 else p
        for d, name in ((-1, "pre == edge - 1"), (0, "pre == edge"), (1, "pre == edge + 1")):
            if edge + d in pres:
                facts.add(name)
        if s.op == OP_ADD2 and any(v >= R for v in pres):
            facts.add("carry out of 2^256")
        if s.op == OP_MUL29_LAZY:
            assert all(v < 2 * p for v in pres), "lazy result not below 2p"
    res = want[:, -8:] if want.shape[1] >= 8 else None
    if res is not None and s.op != OP_PREPARE:
        for v, name in ((0, "result 0"), (1, "result 1"), (p - 1, "result p - 1")):
            if (res == _limbs([v])).all(axis=1).any():
                facts.add(name)
    if s.op == OP_WIDE:
        facts.add(f"top limb max {int(want[:, 16].max())}")
    return sorted(facts)


def run_checks(tasks, workers=8):
    """check_section over tasks on worker processes (spawned: the parent may hold a GPU runtime)"""
    import concurrent.futures
    import multiprocessing
    import os

    workers = max(1, min(workers, os.cpu_count() or 1, len(tasks)))
    if workers == 1:
        return [check_section(t) for t in tasks]
    # the big sections first, so that the pool drains evenly
    order = sorted(range(len(tasks)), key=lambda i: -built(tasks[i][0])[1][tasks[i][1]].n)
    out = [None] * len(tasks)
    with concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as ex:
        for i, r in zip(order, ex.map(check_section, [tasks[i] for i in order])):
            out[i] = r
    return out
