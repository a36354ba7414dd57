"""The definition of the library's multilinear polynomial commitment (zk_mlpcs_commit, zk_mlpcs_open, zk_mlpcs_verify_host,
zk_mlpcs_proof_bytes, zk_mle_eq_sums; the reference has nothing like it, so this file is the definition): BaseFold (Zeilberger, Chen,
Fisch 2023) over the Reed-Solomon code that tests/fri_ref.py folds, in plain Python integers over tests/fri_ref.py, tests/merkle_ref.py,
tests/cmle_ref.py and the C oracle's transcript, and the cases the host and GPU tests share.  Everything is bytes: no tolerance.

  parameters  the field, a table t of 2^n values (n >= 1; variable 0 = the index's top bit), b = log2 of the blowup (1..8), f = log2 of
              the final polynomial's length (0 <= f < n), Q queries (1..1024), a non-zero shift s, a 32-byte seed; R = n - f rounds, every
              fold is by 2; n + b at most the field's two-adicity
  commit      c = cmle_ref.interpolate_fast(t) (key bit v <-> variable v); F_0 = fri_ref.lde(c, n + b, s); one Merkle tree over the two
              column views F_0[0:M_0], F_0[M_0:2 M_0], M_0 = 2^(n+b-1) (layer 0 of fri_ref.prove_evals with a = 1); the commitment is its root
  open at z   z = (z_0 .. z_{n-1}), any elements; v = t(z); transcript: seed; be64 of field id, n, b, f, Q; be32(s); root_0; be32(z_0) ..
              be32(z_{n-1}); be32(v).  T_0 = t, E_0 = eq(., z), claim_0 = v, s_0 = s.  For r = 0 .. R-1: (r >= 1: commit F_r over its two
              column views, absorb root_r); h_r(X) = sum_x' T_r(X, x') E_r(X, x') for X = 0, 1, 2, absorbed as 3 x be32; beta_r =
              sample_field_element; T_{r+1}, E_{r+1} = partial_evaluate(0, [beta_r]); F_{r+1} = fri_ref.fold(F_r, s_r, beta_r, 1);
              s_{r+1} = s_r^2.  A fold by 2 at beta maps the coefficients c[2j], c[2j+1] to c[2j] + beta c[2j+1]: variable 0 again, so
              F_r stays the LDE of the coefficient form of T_r.  final = the first 2^f coefficients of F_R over its coset (the
              coefficient form of T_R), absorbed; the Q query indices as FRI draws them
  proof       h_0 | for r = 1..R-1: root_r, h_r | final | per query, per round r < R: the row (2 x be32), the path (n + b - 1 - r digests);
              layer 0 is opened from the commitment's own tree.  The value v is the public claim, beside the proof
  verify      exact length; canonical elements; the transcript rebuilt; h_r(0) + h_r(1) = claim_r, claim_{r+1} = h_r(beta_r) by the
              quadratic through X = 0, 1, 2; claim_R = (prod_{j<R} eq1(beta_j, z_j)) sum_key final[key] prod_{v in key} z_{R+v}; every
              query as fri_ref.verify does, root_0 the commitment, the betas the sumcheck's, the last fold against final at the query's point
  eq_sums     S_X = sum_{x'} t[X 2^(n-1) + x'] eq(x', tail), X = 0, 1, tail = n - 1 elements: what the device leaves of a round, from which
              h_r(0) = c_r (1 - z_r) S_0, h_r(1) = c_r z_r S_1, h_r(2) = c_r (3 z_r - 1)(2 S_1 - S_0), c_r = prod_{j<r} eq1(beta_j, z_j)"""
import random

import cmle_ref
import fri_ref
import merkle_ref
from oracle import binding as orc

MAX_BLOWUP_LOG, MAX_QUERIES = 8, 1024
# (n, b, f, Q): n = 1..8, b in {1, 2}, every f in {0, 1, 2} below n, Q in {1, 8}
CASES = tuple((n, b, f, q) for n in range(1, 9) for b in (1, 2) for f in (0, 1, 2) if f < n for q in (1, 8))
# what the GPU test adds: layer 0 of 2^12 .. 2^14 points (past the split of FRI's power table), tables past one workgroup of the round
# kernel, sumchecks that pass through every Hi / Lo regime below
GPU_EXTRA_CASES = ((11, 1, 2, 8), (12, 2, 0, 8), (13, 1, 1, 1))
GPU_CASES = tuple(c for c in CASES if c[3] == 8) + GPU_EXTRA_CASES

# ---- the round kernel's shape (zk_amd/csrc/mlpcs_kernels.cuh; tests/test_mlpcs_host.py asserts the arithmetic named here) -------------
# W(x') = eq(x', tail) over m = n - 1 variables is Hi[x' >> L] Lo[x' & (2^L - 1)], L = min(m, LO_BITS): the Lo table in LDS, Hi from
# memory, once per run.  m < RUN_MIN_BITS: one workgroup, one element pair per thread, no Hi.  Otherwise a wave takes a run of 2^S
# elements that share one Hi entry (2^(S-6) trips of 64), S = min(L, max(6, m - RUNS_TARGET_LOG)): as long as the Lo table allows where
# that still leaves 2^RUNS_TARGET_LOG runs.  The grid is min(ceil(2^(m-S) / 4), MAX_BLOCKS) workgroups of four waves and a wave loops
# over runs wave, wave + waves, ...
LO_BITS, RUN_MIN_BITS, RUNS_TARGET_LOG = 9, 6, 11             # kMlLoBits, kMlRunMinBits, kMlRunsTargetLog
THREADS, WAVE, MAX_BLOCKS = 256, 64, 2048                     # kBlock, the wave, kMaxGrid
WAVES_PER_BLOCK = THREADS // WAVE


def run_bits(n):
    """S: log2 of the elements of one run of a table of n variables (run launches only)"""
    m = n - 1
    return min(min(m, LO_BITS), max(RUN_MIN_BITS, m - RUNS_TARGET_LOG))


def runs(n):
    """the runs per half of a table of n variables (run launches only)"""
    return 1 << (n - 1 - run_bits(n))


def blocks(n):
    m = n - 1
    return 1 if m < RUN_MIN_BITS else min(-(-runs(n) // WAVES_PER_BLOCK), MAX_BLOCKS)


def hi_entries(n):
    """entries of the Hi table of a table of n variables: 0 = none (m < L)"""
    m = n - 1
    return 0 if m < LO_BITS else 1 << (m - LO_BITS)


def trips(n):
    """the most runs one wave takes"""
    return -(-runs(n) // (blocks(n) * WAVES_PER_BLOCK))


SECOND_TRIP_VARS = next(n for n in range(1, 41) if trips(n) == 2)   # 24: 2^14 runs of 2^9 on 2^13 waves
# zk_mle_eq_sums on the device against Python integers, n: m = 0; m = 1; both sides of one wave (m = 5: the last launch of one element
# per thread; m = 6: the first run launch, L = m = 6; m = 7); n = L, L + 1, L + 2 (no Hi table, one entry, two), of which the first two
# are also both sides of one workgroup (runs of 64: 4 runs = 4 waves, then 8 = two workgroups); two sizes with many workgroups
EQ_SUMS_VARS = (1, 2, 6, 7, 8, LO_BITS, LO_BITS + 1, LO_BITS + 2, LO_BITS + 3, LO_BITS + 4, 15)
# the same on BN254 against the C oracle's arithmetic: the run lengths between (S = 7, 8 at m = 18, 19; the sizes below all have S = 6),
# the first size with S = 9 below the cap, and the smallest whose launch takes a second trip
ORACLE_SUMS_VARS = (19, 20, 21, SECOND_TRIP_VARS)


def be32(v):
    return int(v).to_bytes(32, "big")


def hash_case(case):
    n, b, f, q = case
    return fri_ref.hash_case((n, b, 1, f, q))


def case_field(case):
    """the field a case runs on, spread as pcs_ref.case_field spreads its cases"""
    return hash_case(case) % 3


def eq1(x, z, p):
    return ((1 - x) * (1 - z) + x * z) % p


def eq_table(z, p):
    """eq(., z) in hypercube order: variable 0 = the index's top bit"""
    out = [1]
    for zj in z:
        out = [e * w % p for e in out for w in ((1 - zj) % p, zj % p)]
    return out


def partial_evaluate0(t, beta, p):
    """partial_evaluate(0, [beta]): the top index bit"""
    h = len(t) // 2
    return [(t[j] + beta * (t[j + h] - t[j])) % p for j in range(h)]


def evaluate(t, z, p):
    for zj in z:
        t = partial_evaluate0(t, zj, p)
    return t[0]


def round_sums(t, e, p):
    """h(X) = sum_x' T(X, x') E(X, x') for X = 0, 1, 2 (zk_round_sums with k = 2, D = 2)"""
    h = len(t) // 2
    out = []
    for x in range(3):
        out.append(sum((t[j] + x * (t[j + h] - t[j])) * (e[j] + x * (e[j + h] - e[j])) for j in range(h)) % p)
    return out


def eq_sums(t, tail, p):
    """(S_0, S_1), S_X = sum_x' t[X 2^(n-1) + x'] eq(x', tail)"""
    h = len(t) // 2
    assert h == 1 << len(tail)
    w = eq_table(tail, p)
    return [sum(t[x * h + j] * w[j] for j in range(h)) % p for x in range(2)]


def sums_to_round(s0, s1, c, z, p):
    """h(0), h(1), h(2) from the two device sums"""
    return [c * (1 - z) * s0 % p, c * z * s1 % p, c * (3 * z - 1) * (2 * s1 - s0) % p]


def quadratic_at(h, x, p):
    """the quadratic through (0, h[0]), (1, h[1]), (2, h[2]) at x"""
    half = pow(2, p - 2, p)
    return (h[0] * (x - 1) * (x - 2) * half - h[1] * x * (x - 2) + h[2] * x * (x - 1) * half) % p


def proof_bytes(n, b, f, q):
    rounds = n - f
    return 32 * (3 * rounds + rounds - 1 + (1 << f)) + 32 * q * sum(2 + n + b - 1 - r for r in range(rounds))


def commit(field, table, b, shift, layer0=None):
    """(F_0, its two column views, the tree's levels); layer0: another F_0 than the table's, what a cheating prover would commit to"""
    p, n = fri_ref.modulus(field), len(table).bit_length() - 1
    assert len(table) == 1 << n and n >= 1
    if layer0 is None:
        nv, coeffs = cmle_ref.interpolate_fast(table, p)
        assert nv == n
        layer0 = fri_ref.lde(field, coeffs, n + b, shift)
    assert len(layer0) == 1 << (n + b)
    m = len(layer0) // 2
    cols = [layer0[:m], layer0[m:]]
    return layer0, cols, merkle_ref.commit(cols)


def _start(field, n, b, f, q, shift, seed, root, z, v):
    assert len(seed) == 32 and len(root) == 32 and len(z) == n
    tr = orc.Transcript()
    tr.append(seed)
    tr.append(b"".join(int(x).to_bytes(8, "big") for x in (field, n, b, f, q)))
    tr.append(be32(shift))
    tr.append(root)
    tr.append(b"".join(be32(x) for x in z))
    tr.append(be32(v))
    return tr


def _query_index(tr, m0):
    return int.from_bytes(tr.sample_challenge()[24:32], "big") & (m0 - 1)


def prove(field, table, b, f, q, shift, seed, z, sumcheck_table=None, layer0=None, committed=None):
    """(v, proof).  sumcheck_table: the sumcheck (and v) run on this table, not on the committed one; layer0: the committed F_0 is this
    one -- two cheating provers.  committed: what commit() returned, when the caller has it"""
    p, n = fri_ref.modulus(field), len(table).bit_length() - 1
    assert 1 <= b <= MAX_BLOWUP_LOG and 0 <= f < n and 1 <= q <= MAX_QUERIES and shift % p
    layer, cols, levels = committed or commit(field, table, b, shift, layer0)
    t = [x % p for x in (sumcheck_table if sumcheck_table is not None else table)]
    z = [x % p for x in z]
    v = evaluate(t, z, p)
    tr = _start(field, n, b, f, q, shift, seed, merkle_ref.root(levels), z, v)
    e, s, rounds = eq_table(z, p), shift, n - f
    layers, trees, out = [cols], [levels], b""
    for r in range(rounds):
        if r >= 1:
            m = len(layer) // 2
            cols = [layer[:m], layer[m:]]
            levels = merkle_ref.commit(cols)
            layers.append(cols)
            trees.append(levels)
            tr.append(merkle_ref.root(levels))
            out += merkle_ref.root(levels)
        h = b"".join(be32(x) for x in round_sums(t, e, p))
        tr.append(h)
        out += h
        beta = orc.to_int(field, tr.sample_field_element(field))
        t, e = partial_evaluate0(t, beta, p), partial_evaluate0(e, beta, p)
        layer = fri_ref.fold(field, layer, s, beta, 1)
        s = s * s % p
    co = fri_ref.fft(field, layer, inverse=True)
    sinv, pw, final = pow(s, p - 2, p), 1, []
    for j in range(1 << f):
        final.append(co[j] * pw % p)
        pw = pw * sinv % p
    fb = b"".join(be32(x) for x in final)
    tr.append(fb)
    out += fb
    m0 = 1 << (n + b - 1)
    for _ in range(q):
        idx = _query_index(tr, m0)
        for r in range(rounds):
            row, path = merkle_ref.open(trees[r], layers[r], idx % (m0 >> r))
            out += b"".join(be32(x) for x in row) + b"".join(path)
    assert len(out) == proof_bytes(n, b, f, q)
    return v, out


def verify(field, n, b, f, q, shift, seed, root, z, v, proof):
    p = fri_ref.modulus(field)
    if len(proof) != proof_bytes(n, b, f, q) or len(z) != n or not 0 <= v < p or any(not 0 <= x < p for x in z):
        return False
    rounds = n - f
    tr = _start(field, n, b, f, q, shift, seed, root, z, v)
    roots, betas, claim, at = [root], [], v, 0

    def elems(count):
        nonlocal at
        got = [int.from_bytes(proof[at + 32 * j:at + 32 * j + 32], "big") for j in range(count)]
        at += 32 * count
        return got

    for r in range(rounds):
        if r >= 1:
            roots.append(proof[at:at + 32])
            tr.append(roots[-1])
            at += 32
        h = elems(3)
        if any(x >= p for x in h) or (h[0] + h[1]) % p != claim:
            return False
        tr.append(proof[at - 96:at])
        betas.append(orc.to_int(field, tr.sample_field_element(field)))
        claim = quadratic_at(h, betas[-1], p)
    final_at = at
    final = elems(1 << f)
    if any(x >= p for x in final):
        return False
    tr.append(proof[final_at:at])
    scale = 1
    for j in range(rounds):
        scale = scale * eq1(betas[j], z[j], p) % p
    if claim != scale * cmle_ref.evaluate_slice(f, final, z[rounds:], p) % p:
        return False
    m0 = 1 << (n + b - 1)
    for _ in range(q):
        idx = _query_index(tr, m0)
        y, s = None, shift
        for r in range(rounds):
            m = m0 >> r
            rho = idx % m
            row = elems(2)
            log_m = m.bit_length() - 1
            path = [proof[at + 32 * j:at + 32 * j + 32] for j in range(log_m)]
            at += 32 * log_m
            if any(x >= p for x in row) or not merkle_ref.verify(roots[r], log_m, 2, rho, row, path):
                return False
            if r > 0 and row[idx // m] != y:
                return False
            x = s * pow(fri_ref.root(field, 2 * m), rho, p) % p
            y = fri_ref.fold(field, row, x, betas[r], 1)[0]
            idx, s = rho, s * s % p
        x = s * pow(fri_ref.root(field, m0 >> (rounds - 1)), idx, p) % p   # N_R = M_{R-1}
        g = 0
        for cj in reversed(final):
            g = (g * x + cj) % p
        if g != y:
            return False
    return True


def section_offsets(n, b, f, q):
    """byte offsets of one element of each section of a proof: an h, a root (None when R = 1), a final coefficient, a row element, a path digest"""
    rounds = n - f
    head = 32 * (3 * rounds + rounds - 1)
    return {"h": 32, "root": 96 if rounds > 1 else None, "final": head, "row": head + (32 << f),
            "path": head + (32 << f) + 64}


def point_entries(p, rng):
    return (0, 1, p - 1, rng.randrange(p))


def case_table(p, field_index, n, worst_case_values):
    """2^n canonical ints from the worst-case limb corpus (fri_ref.fold_input's mix)"""
    return fri_ref.fold_input(p, field_index, n, worst_case_values)


def case_inputs(field_index, case, worst_case_values):
    """(table, shift, seed, z) of a shared case: the table from the worst-case limb corpus, the shift in {1, 5, p - 1, random} and the
    entries of z in {0, 1, p - 1, random} by the case's place"""
    n, b, f, q = case
    p = fri_ref.modulus(field_index)
    rng = random.Random(0x3B5 + 1000 * field_index + hash_case(case))
    table = case_table(p, field_index, n, worst_case_values)
    shift = (1, 5, p - 1, rng.randrange(1, p))[hash_case(case) % 4]
    seed = bytes(rng.randrange(256) for _ in range(32))
    z = [point_entries(p, rng)[(hash_case(case) // 4 + 3 * j) % 4] for j in range(n)]
    return table, shift, seed, z


def eq_sums_case(field_index, n, worst_case_values):
    """(table, tail) of one device zk_mle_eq_sums case: tail entries in {0, 1, p - 1, random}, all four present from n = 8 on"""
    p = fri_ref.modulus(field_index)
    rng = random.Random(0xE95 + 1000 * field_index + n)
    table = case_table(p, field_index, n, worst_case_values)
    tail = [point_entries(p, rng)[(j + n + field_index) % 4] if j % 3 != 2 else rng.randrange(p) for j in range(n - 1)]
    return table, tail
