"""The definition of the library's FRI low-degree proofs (zk_fri_lde, zk_fri_fold, zk_fri_prove, zk_fri_verify_host, zk_fri_proof_bytes;
the reference has no FRI, so this file is the definition), over plain Python integers, the C oracle's Keccak-256 / Transcript /
root_of_unity and tests/merkle_ref.py, and the cases the host and GPU tests share.  Everything is bytes: no tolerance anywhere.

  parameters  the field, d = log2 of the degree bound, b = log2 of the blowup, a = log2 of the fold arity (1..3), f = log2 of the final
              polynomial's length (f < d, a | d - f), Q queries, a non-zero shift, a 32-byte seed; R = (d - f) / a rounds
  domains     layer r: N_r = 2^(d+b-a r) points x_{r,i} = s_r w_r^i in natural order, s_r = shift^(2^(a r)), w_r = root_of_unity(N_r)
  fold2       out[i] = (v[i] + v[i+N/2]) / 2 + beta (v[i] - v[i+N/2]) / (2 s w_N^i), i < N/2
  fold        fold2 a times with (s, beta), (s^2, beta^2), (s^4, beta^4): sum_j beta^j f_j for f(x) = sum_{j<2^a} x^j f_j(x^(2^a))
  lde         coefficients padded to N_0 with zeros, c_j times shift^j, forward transform sum_j c_j w^(j k)
  commit      layer r as 2^a columns of M_r = N_r / 2^a rows, column j = v[j M_r : (j+1) M_r]: row i holds the 2^a inputs of output i
  transcript  seed; be64 of field id, d, b, a, f, Q; be32(shift); per round root_r then beta_r = sample_field_element; the 2^f final
              coefficients as be32; per query idx = int(sample_challenge()[24:32], big endian) & (M_0 - 1)
  query       rho_r = idx mod M_r; open row rho_r of layer r; for r > 0 row[idx_{r-1} div M_r] == y; y = fold(row, x_{r,rho_r}, beta_r, a)[0];
              at the end y == g(x_{R, rho_{R-1}}) for the final polynomial g
  proof       R roots | 2^f coefficients as be32 | per query, per round: the row (2^a x be32), the path (log2 M_r x 32)"""
import random

import merkle_ref
from oracle import binding as orc

FIELD_IDS = ("bn254", "bls12_381", "bls12_377")
SHIFTS = ("one", "five", "minus_one")
# every divisible (d, b, a, f, Q) with d = 2..10, b = 1..3, a = 1..3, f = 0..2, Q in {1, 8}
CASES = tuple((d, b, a, f, q) for d in range(2, 11) for b in (1, 2, 3) for a in (1, 2, 3) for f in (0, 1, 2) if f < d and (d - f) % a == 0
              for q in (1, 8))
# what the GPU test adds: d = 11, 12 (layer 0 of 2^13 .. 2^15 points: past the split of the two-level twiddle table at 2^12)
GPU_EXTRA_CASES = ((11, 1, 3, 2, 8), (11, 2, 1, 1, 1), (12, 1, 2, 0, 8), (12, 3, 3, 0, 8), (12, 2, 1, 2, 1))
GPU_CASES = tuple(c for c in CASES if c[4] == 8 or c[0] <= 4) + GPU_EXTRA_CASES
# zk_fri_fold on the device: log2 N per arity (a single output, a partial wave, one and several workgroups, both sides of the table split)
FOLD_LOGS = (6, 7, 8, 9, 12, 13, 14)


# BN254 only: 2^16 .. 2^14 outputs, 256 .. 64 workgroups of k_fri_fold<a, true>, one 64-element run per wave.  Every output is still
# covered exactly once: the kernel's loop takes a second trip only from 2^24 outputs on (FOLD_BIG below)
FOLD_LOG_LARGE = 17
# (a, log_n, settings of tests/fri_check.py) of the folds whose outputs outnumber the capped grid's 2^23: M = 2^24, two sweeps.  BN254,
# a seeded random table, shift and beta; checked on sampled outputs (fold_at) and against the half-size folds of the even and the odd
# inputs, which do not wrap (tests/test_gpu_fri.py)
FOLD_BIG = ((1, 25, ("fused", "binary")), (3, 27, ("fused",)))
FOLD_BIG_SAMPLES, FOLD_BIG_HALF_SAMPLES = 4096, 256
# (d, b, a, f, Q) of the proofs whose layer 0 has 2^22 points: the tree of round 0 has 2^21 rows at a = 1 (leaves and levels take several
# trips inside zk_fri_prove) and 2^19 at a = 3.  BN254, every setting.
# No case here for the other two kernels.  k_fri_gather over a FRI layer has at most 1024 queries x (8 row elements + 31 siblings) =
# 39,936 items against the 2^19 threads of the capped grid; it does wrap under the polynomial commitment's trace, whose rows have up to
# 1024 elements (513 queries x 1025 items = 525,825): tests/test_gpu_pcs_large.py, pcs_ref.WIDE_MAX_CASE.  k_fri_tables has
# 2^12 + 2^(log_domain - 12) entries, more than 2^19 only from a domain of 2^31 points on (a layer of 64 GiB): no allocatable size wraps.
PROOF_BIG = ((21, 1, 1, 0, 8), (21, 1, 3, 0, 8))


def fold_logs(a):
    return (a, a + 1) + FOLD_LOGS


def fold_combos(log_n):
    """the (shift name, beta index into betas()) pairs a fold of 2^log_n inputs is checked on: all twelve up to 2^9, above that four (two
    at 2^17) that still name every shift and every beta"""
    if log_n <= 9:
        return tuple((s, k) for s in SHIFTS for k in range(4))
    if log_n < FOLD_LOG_LARGE:
        return (("one", 3), ("five", 2), ("minus_one", 1), ("five", 0))
    return (("five", 3), ("minus_one", 2))


def fold_cases(field_index):
    """(a, log_n) of every device fold of one field"""
    return tuple((a, n) for a in (1, 2, 3) for n in fold_logs(a) + ((FOLD_LOG_LARGE,) if field_index == 0 else ()))


def fold_betas(p, field_index, a, log_n):
    return betas(p, random.Random(0xBE7A + 1000 * field_index + 64 * a + log_n))


def modulus(field):
    return orc.modulus(field)


def root(field, n):
    """root_of_unity(n) as a canonical integer"""
    return orc.to_int(field, orc.root_of_unity(field, n))


def be32(v):
    return int(v).to_bytes(32, "big")


def shift_value(p, name):
    return {"one": 1, "five": 5, "minus_one": p - 1}[name]


def betas(p, rng):
    return (0, 1, p - 1, rng.randrange(p))


def fft(field, c, inverse=False):
    """out[k] = sum_j c[j] w^(j k), w = root_of_unity(len(c)) (its inverse and a division by n when inverse)"""
    p, n = modulus(field), len(c)
    if n == 1:
        return list(c)
    w = root(field, n)
    if inverse:
        w = pow(w, p - 2, p)

    def rec(v, w):
        m = len(v)
        if m == 1:
            return v
        ev, od = rec(v[0::2], w * w % p), rec(v[1::2], w * w % p)
        out, t = [0] * m, 1
        for k in range(m // 2):
            x = t * od[k] % p
            out[k], out[k + m // 2] = (ev[k] + x) % p, (ev[k] - x) % p
            t = t * w % p
        return out

    out = rec(list(c), w)
    if inverse:
        ninv = pow(n, p - 2, p)
        out = [x * ninv % p for x in out]
    return out


def fold2(field, v, s, beta):
    p, n = modulus(field), len(v)
    h = n // 2
    winv = pow(root(field, n), p - 2, p)
    cur = pow(2 * s, p - 2, p)   # 1 / (2 s w^i)
    half = pow(2, p - 2, p)
    out = []
    for i in range(h):
        out.append(((v[i] + v[i + h]) * half + beta * (v[i] - v[i + h]) % p * cur) % p)
        cur = cur * winv % p
    return out


def fold(field, v, s, beta, a):
    p = modulus(field)
    for _ in range(a):
        v = fold2(field, v, s, beta)
        s, beta = s * s % p, beta * beta % p
    return v


def fold_at(field, get, log_n, s, beta, a, i):
    """fold(v, s, beta, a)[i] for v of 2^log_n points from the 2^a inputs get(i + j M), M = 2^(log_n - a), alone: fold2's formula applied
    down the recursion (level l of 2^(log_n - l) points under (s^(2^l), beta^(2^l)); its entry idx needs entries idx and idx + half of
    the level below), for layers too large to fold whole in Python"""
    p = modulus(field)
    half = pow(2, p - 2, p)
    # level l - 1 -> l: (s^(2^(l-1)), beta^(2^(l-1)), the root of the 2^(log_n - l + 1) points of the level below)
    consts = [(pow(s, 1 << (l - 1), p), pow(beta, 1 << (l - 1), p), root(field, 1 << (log_n - l + 1))) for l in range(1, a + 1)]

    def rec(l, idx):
        if l == 0:
            return get(idx) % p
        sl, bl, w = consts[l - 1]
        h = 1 << (log_n - l)   # half the level below
        lo, hi = rec(l - 1, idx), rec(l - 1, idx + h)
        cur = pow(2 * sl * pow(w, idx, p), -1, p)   # 1 / (2 s w^idx)
        return ((lo + hi) * half + bl * (lo - hi) % p * cur) % p

    assert 0 <= i < 1 << (log_n - a)
    return rec(a, i)


def fold_big_samples(m, count=FOLD_BIG_SAMPLES):
    """the outputs of a fold with m = 2^24 outputs that are compared with fold_at: the first and the last, both sides of the first
    wave's run, 64 on either side of 2^23 (where the second sweep of the capped grid begins), seeded ones for the rest"""
    idx = {0, 63, 64, m - 1} | set(range((m >> 1) - 64, (m >> 1) + 65))
    rng = random.Random(0xB16 + m)
    while len(idx) < count:
        idx.add(rng.randrange(m))
    return sorted(idx)


def lde(field, coeffs, log_n, shift):
    p, n = modulus(field), 1 << log_n
    assert len(coeffs) <= n
    c, t = [], 1
    for j in range(n):
        c.append(coeffs[j] * t % p if j < len(coeffs) else 0)
        t = t * shift % p
    return fft(field, c)


def proof_bytes(d, b, a, f, q):
    rounds = (d - f) // a
    return 32 * (rounds + (1 << f) + q * sum((1 << a) + (d + b - a * r - a) for r in range(rounds)))


def _start(field, d, b, a, f, q, shift, seed):
    assert len(seed) == 32 and 1 <= a <= 3 and f < d and (d - f) % a == 0 and shift % modulus(field)
    tr = orc.Transcript()
    tr.append(seed)
    tr.append(b"".join(int(v).to_bytes(8, "big") for v in (field, d, b, a, f, q)))
    tr.append(be32(shift))
    return tr


def _query_index(tr, m0):
    return int.from_bytes(tr.sample_challenge()[24:32], "big") & (m0 - 1)


def prove_evals(field, layer0, d, b, a, f, q, shift, seed):
    """the proof bytes, starting from an arbitrary layer 0 of 2^(d+b) canonical integers"""
    p = modulus(field)
    assert len(layer0) == 1 << (d + b)
    tr = _start(field, d, b, a, f, q, shift, seed)
    rounds = (d - f) // a
    v, s = list(layer0), shift
    layers, trees, roots = [], [], []
    for _ in range(rounds):
        m = len(v) >> a
        cols = [v[j * m:(j + 1) * m] for j in range(1 << a)]
        levels = merkle_ref.commit(cols)
        layers.append(cols)
        trees.append(levels)
        roots.append(merkle_ref.root(levels))
        tr.append(roots[-1])
        beta = orc.to_int(field, tr.sample_field_element(field))
        v = fold(field, v, s, beta, a)
        s = pow(s, 1 << a, p)
    co = fft(field, v, inverse=True)
    sinv, t, final = pow(s, p - 2, p), 1, []
    for j in range(1 << f):
        final.append(co[j] * t % p)
        t = t * sinv % p
    tr.append(b"".join(be32(x) for x in final))
    out = b"".join(roots) + b"".join(be32(x) for x in final)
    m0 = len(layer0) >> a
    for _ in range(q):
        idx = _query_index(tr, m0)
        for r in range(rounds):
            rho = idx % (m0 >> (a * r))
            row, path = merkle_ref.open(trees[r], layers[r], rho)
            out += b"".join(be32(x) for x in row) + b"".join(path)
    assert len(out) == proof_bytes(d, b, a, f, q)
    return out


def prove(field, coeffs, d, b, a, f, q, shift, seed):
    assert len(coeffs) <= 1 << d
    return prove_evals(field, lde(field, coeffs, d + b, shift), d, b, a, f, q, shift, seed)


def query_indices(field, proof, d, b, a, f, q, shift, seed):
    """the q indices idx_0 that the transcript of this proof draws (for the tests that plant a change at a queried index)"""
    rounds = (d - f) // a
    tr = _start(field, d, b, a, f, q, shift, seed)
    for r in range(rounds):
        tr.append(proof[32 * r:32 * r + 32])
        tr.sample_field_element(field)
    tr.append(proof[32 * rounds:32 * (rounds + (1 << f))])
    return [_query_index(tr, 1 << (d + b - a)) for _ in range(q)]


def verify(field, proof, d, b, a, f, q, shift, seed):
    p = modulus(field)
    if len(proof) != proof_bytes(d, b, a, f, q):
        return False
    rounds = (d - f) // a
    tr = _start(field, d, b, a, f, q, shift, seed)
    roots, beta = [], []
    for r in range(rounds):
        roots.append(proof[32 * r:32 * r + 32])
        tr.append(roots[-1])
        beta.append(orc.to_int(field, tr.sample_field_element(field)))
    at = 32 * rounds
    final_bytes = proof[at:at + (32 << f)]
    at += 32 << f
    final = [int.from_bytes(final_bytes[32 * j:32 * j + 32], "big") for j in range(1 << f)]
    if any(x >= p for x in final):
        return False
    tr.append(final_bytes)
    m0 = 1 << (d + b - a)
    for _ in range(q):
        idx = _query_index(tr, m0)
        y, s = None, shift
        for r in range(rounds):
            m = m0 >> (a * r)
            rho = idx % m
            row = [int.from_bytes(proof[at + 32 * j:at + 32 * j + 32], "big") for j in range(1 << a)]
            at += 32 << a
            log_m = m.bit_length() - 1
            path = [proof[at + 32 * j:at + 32 * j + 32] for j in range(log_m)]
            at += 32 * log_m
            if any(x >= p for x in row):
                return False
            if not merkle_ref.verify(roots[r], log_m, 1 << a, rho, row, path):
                return False
            if r > 0 and row[idx // m] != y:
                return False
            x = s * pow(root(field, m << a), rho, p) % p
            y = fold(field, row, x, beta[r], a)[0]
            idx, s = rho, pow(s, 1 << a, p)
        x = s * pow(root(field, m0 >> (a * (rounds - 1))), idx, p) % p   # N_R = M_{R-1}
        g = 0
        for cj in reversed(final):
            g = (g * x + cj) % p
        if g != y:
            return False
    return True


def case_inputs(field_index, case):
    """(coefficients, shift, seed) of a shared case: 2^d - 1, 2^d or fewer coefficients, the shift by the case's place in the list"""
    d, b, a, f, q = case
    p = modulus(field_index)
    rng = random.Random(0xF41 + 1000 * field_index + hash_case(case))
    n = (1 << d) - (rng.randrange(3) % 2)
    coeffs = [rng.randrange(p) for _ in range(n)]
    coeffs[0], coeffs[-1] = p - 1, rng.randrange(1, p)
    shift = (1, 5, p - 1, rng.randrange(1, p))[hash_case(case) % 4]
    seed = bytes(rng.randrange(256) for _ in range(32))
    return coeffs, shift, seed


def hash_case(case):
    d, b, a, f, q = case
    return ((((d * 4 + b) * 4 + a) * 4 + f) * 16 + q)


def case_field(case):
    """the field a case runs on where a test takes one field per case"""
    return hash_case(case) % 3


def fold_input(p, field_index, log_n, worst_case_values):
    """2^log_n canonical ints: seeded random values mixed with the worst-case limb patterns of tests/field_corpus.py, zeros and p - 1"""
    rng = random.Random(0xF01D + 1000 * field_index + log_n)
    worst = worst_case_values(p, field_index, 256) + [0, 0, p - 1, p - 1]
    v = [rng.choice(worst) if rng.random() < 0.3 else rng.randrange(p) for _ in range(1 << log_n)]
    v[0], v[-1] = 0, p - 1
    return v
