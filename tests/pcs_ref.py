"""The definition of the library's FRI polynomial commitment (zk_deep_quotient, zk_pcs_commit, zk_pcs_open, zk_pcs_verify_host,
zk_pcs_proof_bytes; the reference has nothing like it, so this file is the definition), over plain Python integers, tests/fri_ref.py,
tests/merkle_ref.py and the C oracle's transcript, and the cases the host and GPU tests share.  Everything is bytes: no tolerance.

  parameters  the field, k >= 1 polynomials of at most 2^d coefficients, d, b, a, f, Q with FRI's meaning and limits, k 2^a <= 1024, a
              non-zero shift s, a 32-byte seed; N = 2^(d+b), M = N / 2^a, w = root_of_unity(N), x_i = s w^i
  commit      F_c = fri_ref.lde(f_c, d + b, s); one Merkle tree of M rows over the k 2^a column views, column c 2^a + j = F_c[j M : (j+1) M]
              (FRI's own row layout: row i holds every value the verifier needs at FRI query index i); the commitment is the root
  open at z   z off the domain (z^N != s^N); y_c = f_c(z); transcript: seed; be64 of field id, k, d, b, a, f, Q; be32(s); root; be32(z);
              be32(y_0) .. be32(y_{k-1}); alpha = sample_field_element; fri_seed = sample_challenge()
              q[i] = (sum_c alpha^c (F_c[i] - y_c)) / (x_i - z): fewer than 2^d coefficients exactly when every y_c is right
              FRI part = fri_ref.prove_evals(x_i q[i], d, b, a, f, Q, s, fri_seed) with the query indices idx_t of that part
  proof       the FRI part | per query t: row idx_t of the commitment tree (k 2^a x be32), its path ((d + b - a) x 32 bytes); the values
              y are the public claim, beside the proof
  verify      exact length; canonical elements; fri_ref.verify of the FRI part under fri_seed; every tree opening; for every j < 2^a entry j
              of the FRI part's round-0 row of query t equals x (sum_c alpha^c (row[c 2^a + j] - y_c)) / (x - z) at x = x_{idx_t + j M}
  bound       FRI's bound is 2^d coefficients, one more than q may have: q of an f_c with 2^d + 1 coefficients has exactly 2^d and would
              pass.  So the layer FRI sees is X q(X), which has at most 2^d coefficients exactly when q has at most 2^d - 1, that is when
              every f_c has at most 2^d (tests/test_pcs_host.py has both sides); zk_deep_quotient itself is the plain q"""
import random

import numpy as np

import fri_ref
import merkle_ref
from oracle import binding as orc

MAX_COLUMNS = 1024
# (k, d, b, a, f, Q): every divisible shape with k in {1, 2, 5}, d = 3..8, b in {1, 2}, a in {1, 2, 3}, f in {0, 1}, Q in {1, 8}
CASES = tuple((k, d, b, a, f, q) for k in (1, 2, 5) for d in range(3, 9) for b in (1, 2) for a in (1, 2, 3) for f in (0, 1) if (d - f) % a == 0
              for q in (1, 8))
# what the GPU test adds: layer 0 of 2^12 .. 2^14 points (one chunk of the quotient kernel is 2^11, the split of its power table 2^12)
GPU_EXTRA_CASES = ((2, 11, 1, 3, 2, 8), (3, 12, 2, 2, 0, 8), (1, 12, 1, 1, 1, 1))
GPU_CASES = tuple(c for c in CASES if c[5] == 8) + GPU_EXTRA_CASES
# zk_deep_quotient on the device: log2 N (one output, a partial wave, one and two waves, exactly one chunk, two chunks = the split of
# the power table, more) and the numbers of columns
QUOTIENT_LOGS = (1, 3, 6, 7, 11, 12, 13, 14)
QUOTIENT_COLUMNS = (1, 2, 3, 5, 17)
SHIFTS = fri_ref.SHIFTS
# The launch covers its outputs with one workgroup per chunk of 2^11 (no capped grid, no loop): every output is written by exactly one
# thread at every size, so there is no sweep boundary to test.  A grid of more than 2^31 - 1 workgroups is refused; that is 2^42
# outputs, past the largest table (2^40) and any allocatable size.


# ---- the shapes of tests/test_gpu_pcs_large.py (child: tests/pcs_large_check.py): the first further trip of every loop and second-level
# launch on the commitment's path.  The lists above stay as they are; tests/test_pcs_large_host.py asserts the arithmetic named here.
PTR_BATCH, CHUNK, TOTALS_THREADS = 32, 1 << 11, 256           # pcs_kernels.cuh kPcsPtrBatch, kPcsChunk, kBlock (k_pcs_totals: one workgroup)
EVAL_RUN, EVAL_THREADS, EVAL_MAX_BLOCKS = 16, 256, 64         # pcs_kernels.cuh kPcsEvalRun, kBlock, kPcsEvalMaxBlocks
GATHER_THREADS = 2048 * 256                                   # host_core.hpp grid_for: at most 2048 workgroups of 256 = 2^19 threads
# A. wide quotients: quotient_plan sends the column pointers 32 per k_pcs_put_ptrs launch, so k = 32 is one full batch, 33 the first
# launch with base > 0 (one pointer), 64 two full ones, 65 three; 1024 = MAX_COLUMNS is 32 launches.  log2 N = 3: !RUN (N < 64);
# 6: ALONE + RUN; 12: two chunks = three launches, at the split of the power table
WIDE_QUOTIENT_COLUMNS = (32, 33, 64, 65)
WIDE_QUOTIENT_LOGS = (3, 6, 12)
WIDE_QUOTIENT_MAX = (6, MAX_COLUMNS)
# A. wide openings, (field index, (k, d, b, a, f, Q)): widths k 2^a = 66 and 72 (three pointer batches, in Merkle leaves of 66 and 72
# columns) and 1024, the widest the ABI accepts, on every field.  The last one's trace gather has Q (width + log2 M) = 513 (1024 + 1) =
# 525,825 items against the 524,288 threads of the capped grid: k_fri_gather's loop takes a second trip for the last 1,537 of them
WIDE_MAX_CASE = (128, 3, 1, 3, 0, 513)
WIDE_CASES = ((0, (33, 4, 1, 1, 0, 8)), (1, (9, 5, 2, 3, 2, 8)), (0, WIDE_MAX_CASE), (1, WIDE_MAX_CASE), (2, WIDE_MAX_CASE))
WIDE_VERIFY_FIELD = 2   # the field on which pcs_ref.verify reads the 17 MB proof of WIDE_MAX_CASE too (2.2 s)
# B. mid openings: k_pcs_eval_partial runs min(ceil(2^d / 4096), 64) workgroups per polynomial, so d = 13, 14, 15 are the first with 2, 4
# and 8 partials per polynomial (gridDim.x > 1, z^j0 with j0 >= 4096, k_pcs_eval_final adding several); on every setting of the switch
MID_CASES = ((0, (2, 13, 1, 1, 0, 8)), (1, (3, 14, 1, 3, 2, 8)), (2, (1, 15, 1, 2, 1, 1)))
# B. the quotient sizes missing between the tested ones: N = 1 (log_n = 0, lo_bits = 0, w = 1: the domain is the one point s), 2^5 (the
# largest !RUN launch), 2^9 (ALONE with the rows q = 2 .. 7 of every thread wholly outside)
EDGE_QUOTIENT_LOGS = (0, 5, 9)
EDGE_QUOTIENT_COLUMNS = (1, 2, 3)
# C. big, BN254 only.  (log_n, k) of the quotients: N / 2^11 = 512 and 1024 chunk products on k_pcs_totals' 256 threads, 2 and 4 per
# thread (the halves of the first, 2^19 points, are 256 chunks: one per thread, every thread busy).  The opening: 2^19 / 16 = 32,768 runs
# of coefficients per polynomial against 64 x 256 = 16,384 threads, two trips of k_pcs_eval_partial's loop, 64 partials per polynomial,
# and a quotient of 2^20 points through the TIMES_X variant
BIG_QUOTIENTS = ((20, 3), (21, 1))
BIG_SAMPLES, BIG_HALF_SAMPLES = 4096, 256
BIG_CASE = (2, 19, 1, 3, 1, 8)


def totals_per_thread(log_n):
    """the chunk products one thread of k_pcs_totals takes: ceil((N / 2^11) / 256)"""
    return -(-((1 << log_n) // CHUNK) // TOTALS_THREADS)


def eval_partials(d):
    """the workgroups (= partial sums) per polynomial of k_pcs_eval_partial: min(ceil(2^d / (256 x 16)), 64)"""
    return min(-(-(1 << d) // (EVAL_THREADS * EVAL_RUN)), EVAL_MAX_BLOCKS)


def gather_items(case):
    """the items of the opening's trace gather: per query a row of k 2^a elements and a path of log2 M digests"""
    k, d, b, a, f, q = case
    return q * ((k << a) + d + b - a)


def be32(v):
    return int(v).to_bytes(32, "big")


def hash_case(case):
    k, d, b, a, f, q = case
    return fri_ref.hash_case((d, b, a, f, q)) * 8 + k


def case_field(case):
    """the field a case runs on, spread as fri_ref.case_field spreads its cases"""
    return hash_case(case) % 3


def on_domain(field, log_n, s, z):
    p = fri_ref.modulus(field)
    return pow(z, 1 << log_n, p) == pow(s, 1 << log_n, p)


def _domain_root(field, n):
    return 1 if n == 1 else fri_ref.root(field, n)


def evaluate(field, coeffs, z):
    p, y = fri_ref.modulus(field), 0
    for cj in reversed(coeffs):
        y = (y * z + cj) % p
    return y


def quotient_at(field, get, k, log_n, s, z, ys, alpha, i):
    """q[i] alone from the k values get(c, i), for tables too large to compute whole in Python"""
    p = fri_ref.modulus(field)
    x = s * pow(_domain_root(field, 1 << log_n), i, p) % p
    num, t = 0, 1
    for c in range(k):
        num = (num + t * (get(c, i) - ys[c])) % p
        t = t * alpha % p
    return num * pow((x - z) % p, p - 2, p) % p


def quotient(field, columns, s, z, ys, alpha):
    """q[i] = (sum_c alpha^c (columns[c][i] - ys[c])) / (s w^i - z) over the N = len(columns[0]) points of the coset"""
    p, n = fri_ref.modulus(field), len(columns[0])
    assert n & (n - 1) == 0 and all(len(col) == n for col in columns) and len(ys) == len(columns)
    assert not on_domain(field, n.bit_length() - 1, s, z)
    w, x, dens = _domain_root(field, n), s % p, []
    for i in range(n):
        dens.append((x - z) % p)
        x = x * w % p
    # the inverses by Montgomery's trick (a field inverse is unique: the same integers as pow(den, p - 2, p) one by one)
    pre, acc = [], 1
    for den in dens:
        pre.append(acc)
        acc = acc * den % p
    back, out = pow(acc, p - 2, p), [0] * n
    for i in reversed(range(n)):
        num = 0
        for c in reversed(range(len(columns))):   # Horner over the columns
            num = (num * alpha + columns[c][i] - ys[c]) % p
        out[i] = num * (back * pre[i] % p) % p
        back = back * dens[i] % p
    return out


def times_x(field, quo, s):
    """x_i quo[i]: the evaluations of X q(X) over the coset"""
    p, n = fri_ref.modulus(field), len(quo)
    w, x, out = _domain_root(field, n), s % p, []
    for v in quo:
        out.append(v * x % p)
        x = x * w % p
    return out


def proof_bytes(k, d, b, a, f, q):
    return fri_ref.proof_bytes(d, b, a, f, q) + 32 * q * ((k << a) + d + b - a)


def commit(field, polys, d, b, a, shift):
    """(the LDEs F_c, the column views, the tree's levels)"""
    assert polys and (len(polys) << a) <= MAX_COLUMNS
    m = 1 << (d + b - a)
    ldes = [fri_ref.lde(field, co, d + b, shift) for co in polys]
    cols = [F[j * m:(j + 1) * m] for F in ldes for j in range(1 << a)]
    return ldes, cols, merkle_ref.commit(cols)


def _challenges(field, k, d, b, a, f, q, shift, seed, root, z, ys):
    assert len(seed) == 32 and len(root) == 32
    tr = orc.Transcript()
    tr.append(seed)
    tr.append(b"".join(int(v).to_bytes(8, "big") for v in (field, k, d, b, a, f, q)))
    tr.append(be32(shift))
    tr.append(root)
    tr.append(be32(z))
    tr.append(b"".join(be32(y) for y in ys))
    alpha = orc.to_int(field, tr.sample_field_element(field))
    return alpha, tr.sample_challenge()


def prove(field, polys, d, b, a, f, q, shift, seed, z, ys=None, committed=None):
    """(values, proof).  The polynomials may be longer than 2^d (up to 2^(d+b)) and ys may be given: what a cheating prover would send.
    committed: what commit() returned for these polynomials, when the caller has it."""
    k = len(polys)
    ldes, cols, levels = committed or commit(field, polys, d, b, a, shift)
    assert not on_domain(field, d + b, shift, z)
    if ys is None:
        ys = [evaluate(field, co, z) for co in polys]
    alpha, fri_seed = _challenges(field, k, d, b, a, f, q, shift, seed, merkle_ref.root(levels), z, ys)
    quo = times_x(field, quotient(field, ldes, shift, z, ys, alpha), shift)
    out = fri_ref.prove_evals(field, quo, d, b, a, f, q, shift, fri_seed)
    for idx in fri_ref.query_indices(field, out, d, b, a, f, q, shift, fri_seed):
        row, path = merkle_ref.open(levels, cols, idx)
        out += b"".join(be32(x) for x in row) + b"".join(path)
    assert len(out) == proof_bytes(k, d, b, a, f, q)
    return list(ys), out


def verify(field, k, d, b, a, f, q, shift, seed, root, z, ys, proof):
    p = fri_ref.modulus(field)
    assert not on_domain(field, d + b, shift, z)
    if len(proof) != proof_bytes(k, d, b, a, f, q) or len(ys) != k or any(not 0 <= y < p for y in ys):
        return False
    alpha, fri_seed = _challenges(field, k, d, b, a, f, q, shift, seed, root, z, ys)
    fri_len = fri_ref.proof_bytes(d, b, a, f, q)
    fri_part = proof[:fri_len]
    if not fri_ref.verify(field, fri_part, d, b, a, f, q, shift, fri_seed):
        return False
    rounds, log_m, width = (d - f) // a, d + b - a, k << a
    m, w = 1 << log_m, fri_ref.root(field, 1 << (d + b))
    per_query = fri_ref.proof_bytes(d, b, a, f, 1) - 32 * (rounds + (1 << f))
    at = fri_len
    for t, idx in enumerate(fri_ref.query_indices(field, fri_part, d, b, a, f, q, shift, fri_seed)):
        row = [int.from_bytes(proof[at + 32 * j:at + 32 * j + 32], "big") for j in range(width)]
        at += 32 * width
        path = [proof[at + 32 * j:at + 32 * j + 32] for j in range(log_m)]
        at += 32 * log_m
        if any(x >= p for x in row) or not merkle_ref.verify(root, log_m, width, idx, row, path):
            return False
        r0 = 32 * (rounds + (1 << f)) + t * per_query   # the FRI part's round-0 row of this query
        for j in range(1 << a):
            x = shift * pow(w, idx + j * m, p) % p
            want = x * quotient_at(field, lambda c, i: row[(c << a) + j], k, d + b, shift, z, ys, alpha, idx + j * m) % p
            if int.from_bytes(fri_part[r0 + 32 * j:r0 + 32 * j + 32], "big") != want:
                return False
    return True


def case_inputs(field_index, case):
    """(polynomials, shift, seed, z) of a shared case: 2^d, 2^d - 1 or fewer coefficients, the shift and z by the case's place"""
    k, d, b, a, f, q = case
    p = fri_ref.modulus(field_index)
    rng = random.Random(0x9C5 + 1000 * field_index + hash_case(case))
    polys = []
    for c in range(k):
        n = (1 << d) - (c % 3 if c % 3 < 2 else rng.randrange(1 << d))
        co = [rng.randrange(p) for _ in range(n)]
        co[0], co[-1] = p - 1, rng.randrange(1, p)
        polys.append(co)
    shift = (1, 5, p - 1, rng.randrange(1, p))[hash_case(case) % 4]
    seed = bytes(rng.randrange(256) for _ in range(32))
    z = (0, rng.randrange(p), p - 1, rng.randrange(p))[(hash_case(case) // 4) % 4] if shift != p - 1 else rng.randrange(p)
    while on_domain(field_index, d + b, shift, z):
        z = rng.randrange(p)
    return polys, shift, seed, z


def quotient_points(p, rng):
    """the four z and the four alpha of the device quotient cases"""
    return (0, 1, p - 1, rng.randrange(p))


def quotient_combos(log_n, k):
    """(shift name, z index, alpha index) a quotient of 2^log_n points over k columns is checked on: all 48 up to 2^7 points with k <= 3,
    above that four that still name every shift, every z and every alpha (thinned as fri_ref.fold_combos thins the folds)"""
    if log_n <= 7 and k <= 3:
        return tuple((s, zi, ai) for s in SHIFTS for zi in range(4) for ai in range(4))
    return (("one", 3, 0), ("five", 1, 1), ("minus_one", 0, 2), ("five", 2, 3))   # (1 and p - 1 lie off the coset of 5 only)


def quotient_sizes(field_index):
    """(log_n, k) of every device quotient of one field, thinned so that every size and every number of columns still appears: BN254
    takes the whole product up to two chunks (2^12) and two numbers of columns above; the other two fields every size with one number
    of columns, rotating over the list, and 17 columns at two chunks"""
    if field_index == 0:
        large = {13: (2, 17), 14: (1, 5)}
        return tuple((n, k) for n in QUOTIENT_LOGS for k in large.get(n, QUOTIENT_COLUMNS))
    picked = tuple((n, QUOTIENT_COLUMNS[(i + field_index) % len(QUOTIENT_COLUMNS)]) for i, n in enumerate(QUOTIENT_LOGS))
    return picked + ((12, 17),)


def quotient_case(field_index, log_n, k, shift_name, zi, ai):
    """(s, z, alpha, ys) of one device quotient; a z that falls on the domain (0 never does; 1 and p - 1 do for shifts 1 and p - 1) is
    replaced by a seeded one off it"""
    p = fri_ref.modulus(field_index)
    rng = random.Random(0xDEE9 + 1000 * field_index + 64 * log_n + k)
    zs, alphas = quotient_points(p, rng), quotient_points(p, rng)
    s, z = fri_ref.shift_value(p, shift_name), zs[zi]
    while on_domain(field_index, log_n, s, z):
        z = rng.randrange(p)
    ys = [rng.randrange(p) for _ in range(k)]
    ys[0] = p - 1
    return s, z, alphas[ai], ys


THINNED_COMBOS = quotient_combos(8, 1)   # the four above 2^7 points, for the wide and the edge shapes at every size


def wide_quotient_sizes(field_index):
    """(log_n, k) of the wide device quotients of one field: BN254 the whole product and 1024 columns, the other two fields the two
    numbers of columns that open a further pointer batch at two chunks, and 1024"""
    if field_index == 0:
        return tuple((n, k) for n in WIDE_QUOTIENT_LOGS for k in WIDE_QUOTIENT_COLUMNS) + (WIDE_QUOTIENT_MAX,)
    return ((12, 33), (12, 65), WIDE_QUOTIENT_MAX)


def edge_quotient_sizes(field_index):
    return tuple((n, k) for n in EDGE_QUOTIENT_LOGS for k in EDGE_QUOTIENT_COLUMNS)


def quotient_big_samples(log_n, count=BIG_SAMPLES):
    """the outputs of a quotient of N = 2^log_n points that are compared with quotient_at: the first and the last, both sides of the
    first wave's run, of the first chunk and of the split of the power table, both sides of every run boundary 2048 per t of
    k_pcs_totals (thread t starts at chunk t per) for t in {1, 2, 128, 255, 256}, seeded ones for the rest"""
    n = 1 << log_n
    idx = {0, n - 1, 63, 64, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK}
    for b in quotient_run_boundaries(log_n):
        idx |= {b - 1, b}
    idx = {i for i in idx if 0 <= i < n}
    rng = random.Random(0xB16 + 4 * log_n + (count == BIG_SAMPLES))
    while len(idx) < count:
        idx.add(rng.randrange(n))
    return sorted(idx)


def quotient_run_boundaries(log_n):
    """the first output of thread t's run of chunk products in k_pcs_totals, t in {1, 2, 128, 255, 256} (256: one past the last)"""
    return tuple(CHUNK * totals_per_thread(log_n) * t for t in (1, 2, 128, 255, 256))


def lde_by_oracle(field, coeffs, log_n, shift):
    """fri_ref.lde by the C oracle's transform, for sizes fri_ref.fft takes too long at: the (2^log_n, 4) Montgomery elements
    (tests/test_pcs_large_host.py holds the two equal at small sizes)"""
    p, n = fri_ref.modulus(field), 1 << log_n
    assert len(coeffs) <= n
    scaled, t = [], 1
    for cj in coeffs:
        scaled.append(cj * t % p)
        t = t * shift % p
    src = np.zeros((n, 4), dtype=np.uint64)
    src[:len(scaled)] = orc.from_ints(field, scaled)
    return orc.ntt_fast(field, src)


def big_quotient_inputs(log_n, k):
    """(s, z, alpha, ys) of a big quotient on BN254: seeded, z off the domain"""
    p = fri_ref.modulus(0)
    rng = random.Random(0xB16DEE9 + 64 * log_n + k)
    s, z, alpha = rng.randrange(1, p), rng.randrange(p), rng.randrange(p)
    while on_domain(0, log_n, s, z):
        z = rng.randrange(p)
    return s, z, alpha, [rng.randrange(p) for _ in range(k)]


def big_case_inputs():
    """(shift, seed, z, another z) of BIG_CASE on BN254; both points off the domain"""
    k, d, b, a, f, q = BIG_CASE
    p = fri_ref.modulus(0)
    rng = random.Random(0xB16 + hash_case(BIG_CASE))
    shift = rng.randrange(1, p)
    seed = bytes(rng.randrange(256) for _ in range(32))
    zs = []
    while len(zs) < 2:
        z = rng.randrange(p)
        if not on_domain(0, d + b, shift, z) and z not in zs:
            zs.append(z)
    return shift, seed, zs[0], zs[1]


def quotient_columns(p, field_index, log_n, k, worst_case_values):
    """k columns from fri_ref.fold_input's generator (worst-case limb corpus), column c rotated by c so that no two are equal"""
    base = fri_ref.fold_input(p, field_index, log_n, worst_case_values)
    return [base[c % len(base):] + base[:c % len(base)] for c in range(k)]
