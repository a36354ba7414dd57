"""The definition of the library's fractional-sum (LogUp) argument and of its lookup multiplicities (zk_mle_fraction_tree, zk_fsum_prove,
zk_fsum_verify_host, zk_fsum_proof_bytes, zk_lookup_multiplicities; the reference has nothing like them, so this file is the definition):
N / D = sum_i p[i] / (q[i] + sigma) by a binary tree of fractions whose layers are tied together by one degree-3 sumcheck each, all on one
transcript, in plain Python integers over the C oracle's transcript, and the cases the host and GPU tests share.  Everything is bytes: no
tolerance.  Every convention not restated here is tests/gprod_ref.py's: variable 0 = the index's top bit, be32, the round evaluations at
X = 0, 1, 2, 3, partial_evaluate(0, ..) folds.

  parameters  the field, q: a table of 2^n values (1 <= n <= 40), p: a table of 2^n values or None = all ones, a shift sigma (None = 0, the
              same bytes as an explicit 0), a 32-byte seed
  tree        P_n[i] = p[i] (1 when p is None), Q_n[i] = q[i] + sigma; for i < 2^j: P_j[i] = P_{j+1}[i] Q_{j+1}[i + 2^j] + P_{j+1}[i + 2^j]
              Q_{j+1}[i], Q_j[i] = Q_{j+1}[i] Q_{j+1}[i + 2^j]; N = P_0[0], D = Q_0[0].  fraction_tree() is the two heaps the device call
              returns: heapP[0] = 0, heapQ[0] = 1, heap[2^j + i] = level j (j < n); heapQ is gprod_ref.product_tree(q, sigma).  Nothing is
              inverted: a zero denominator gives D = 0, not an error
  transcript  orc.Transcript(); the seed; be64(field id), be64(n), be64(1 if p is given else 0); be32(sigma); be32(N), be32(D)
  layers      j = 0 .. n-1, each the claims (cP_j, cQ_j) = (P_j(r_j), Q_j(r_j)) at a point r_j of j elements; r_0 = (), (cP_0, cQ_0) = (N, D).
              For j >= 1: lambda_j = sample_field_element; absorb be32(cP_j + lambda_j cQ_j); the sumcheck of j rounds on sum_x eq(x, r_j)
              [P0(x) Q1(x) + P1(x) Q0(x) + lambda_j Q0(x) Q1(x)], X0 / X1 the low / high half of level j + 1: each round sends h at
              X = 0, 1, 2, 3 (absorbed as 4 x be32), rho_i = sample_field_element, every table folded.  At the end of every layer (j = 0
              too, where they are the four entries of level 1): p0, p1, q0, q1 = P0(rho), P1(rho), Q0(rho), Q1(rho), absorbed as 4 x be32;
              tau_j = sample_field_element; r_{j+1} = (tau_j, rho); cP_{j+1} = p0 + tau_j (p1 - p0), cQ_{j+1} likewise
  proof       per layer the 4 j round evaluations, then the four values: 2 n^2 + 2 n elements of 32 bytes.  (N, D) is the public claim
  verify      exact length; every element, N and D canonical (else False, not an error); D = 0 gives False (D is the product of all
              denominators, so D != 0 is what makes the sum well defined); layer 0: N = p0 q1 + p1 q0, D = q0 q1; layer j >= 1, per round
              h(0) + h(1) = claim and the new claim is the cubic at rho_i, at the end claim = eq(r_j, rho) (p0 q1 + p1 q0 + lambda_j q0 q1);
              with p = None also cP_n = 1.  The output is the point r_n and (cP_n, cQ_n - sigma), which the caller checks as p(r_n), q(r_n)
  binding     as gprod_ref: the tables are not absorbed, the seed must bind them; a sigma used as a challenge is drawn after that

  multiplicities(table, witness)   (m, missing, first_missing, duplicates), see the function
  lookup_prove / lookup_verify     the lookup composition made of the calls above only, see the functions"""
import random

from oracle import binding as orc

import gprod_ref as gp
from gprod_ref import be32, cubic_at, eq_table, evaluate, partial_evaluate0  # noqa: F401  (the tests use them through this module)

MAX_VARS = gp.MAX_VARS
# ---- the kernels' shape (zk_amd/csrc/fsum_kernels.cuh, fsum.hip; tests/test_fsum_host.py matches the constants named here) ---------------
# The tree follows gprod_ref's: levels above 2^LDS_VARS elements are taken down FUSE levels per launch (k_ftree<A>), then one workgroup
# finishes levels LDS_VARS .. 0 out of LDS (k_ftree_lds), one thread per element of a fused launch's lowest level on a grid capped at
# MAX_BLOCKS_STREAM workgroups.  The count kernel of the multiplicities has one thread per witness entry on a grid capped at MAX_BLOCKS.
LDS_VARS = 10                                   # kFtreeLdsVars
FUSE_MAX, FUSE_DEFAULT = 2, 2                   # kFtreeMaxFuse, kFtreeFuseDefault
THREADS, MAX_BLOCKS_STREAM, MAX_BLOCKS = gp.THREADS, gp.MAX_BLOCKS_STREAM, 2048   # kBlock, kMaxGridStream, kMaxGrid
MULT_MAX_TABLE_VARS, MULT_MAX_WITNESS_VARS = 30, 31   # kMultMaxTableVars, kMultMaxWitnessVars
NONE_MISSING = (1 << 64) - 1


def launches(n, fuse=FUSE_DEFAULT):
    """[(A, m)]: the fused launches of a tree over 2^n values, each taking level m + A to levels m + A - 1 .. m"""
    out, top = [], n
    while top > LDS_VARS:
        a = min(fuse, top - LDS_VARS)
        out.append((a, top - a))
        top -= a
    return out


def trips(n, fuse=FUSE_DEFAULT):
    """the most runs of 64 elements one wave of the first (largest) fused launch takes; 0 = no fused launch"""
    ls = launches(n, fuse)
    if not ls:
        return 0
    threads = 1 << ls[0][1]
    return -(-threads // (min(-(-threads // THREADS), MAX_BLOCKS_STREAM) * THREADS))


# the smallest n at which the capped grid's loop takes a second trip, per switch setting
SECOND_TRIP_VARS = {f: next(n for n in range(1, MAX_VARS + 1) if trips(n, f) == 2) for f in range(1, FUSE_MAX + 1)}
# the smallest witness at which a thread of the count kernel takes a second entry
MULT_SECOND_TRIP_VARS = next(n for n in range(MULT_MAX_WITNESS_VARS + 1) if (1 << n) > MAX_BLOCKS * THREADS)

SHIFT_KINDS = gp.SHIFT_KINDS
# (n, variant, special): n = 1..8 in two variants -- variant 0 with p given, variant 1 with p = None; "cancel": q[i] + sigma = 0 for one i
CASES = tuple((n, v, "") for n in range(1, 9) for v in (0, 1)) + ((6, 2, "cancel"),)
# what the GPU test adds: 1 .. 4 levels above the LDS stage (every arity, then two launches); p given on the even sizes
GPU_EXTRA_CASES = tuple((LDS_VARS + k, 3, "") for k in (1, 2, 3, 4))
GPU_CASES = CASES + GPU_EXTRA_CASES
TREE_VARS = tuple(range(1, LDS_VARS + 3))


def hash_case(case):
    n, v, special = case
    return (2 * n + v) * 7 + 3 + len(special)


def case_field(case):
    return case[0] % 3 if case[1] == 3 else (hash_case(case) // 5) % 3


def case_shift_kind(case):
    return "random" if case[2] == "cancel" else SHIFT_KINDS[hash_case(case) % 5]


def case_has_p(case):
    n, v, special = case
    return n % 2 == 0 if v == 3 else v != 1


def proof_bytes(n):
    return 64 * n * (n + 1)


def tree(q, p_tab, shift, p):
    """([P_0 .. P_n], [Q_0 .. Q_n])"""
    n = len(q).bit_length() - 1
    assert len(q) == 1 << n and n >= 1 and (p_tab is None or len(p_tab) == len(q))
    P = [[x % p for x in p_tab] if p_tab is not None else [1] * len(q)]
    Q = [[(x + (shift or 0)) % p for x in q]]
    for j in range(n - 1, -1, -1):
        up_p, up_q, h = P[0], Q[0], 1 << j
        P.insert(0, [(up_p[i] * up_q[i + h] + up_p[i + h] * up_q[i]) % p for i in range(h)])
        Q.insert(0, [up_q[i] * up_q[i + h] % p for i in range(h)])
    return P, Q


def fraction_tree(q, p_tab, shift, p):
    """the two heaps zk_mle_fraction_tree returns: 2^n elements each"""
    P, Q = tree(q, p_tab, shift, p)
    return [0] + [x for level in P[:-1] for x in level], [1] + [x for level in Q[:-1] for x in level]


def _start(field, n, has_p, shift, seed):
    assert len(seed) == 32
    tr = orc.Transcript()
    tr.append(bytes(seed))
    tr.append(int(field).to_bytes(8, "big") + int(n).to_bytes(8, "big") + int(1 if has_p else 0).to_bytes(8, "big"))
    tr.append(be32(shift or 0))
    return tr


_sample = gp._sample


def _lin(t, x, h, j):
    return t[j] + x * (t[j + h] - t[j])


def round_evals(e, p0, p1, q0, q1, lam, p):
    """h(X) = sum_x' E [P0 Q1 + P1 Q0 + lambda Q0 Q1](X, x') at X = 0, 1, 2, 3"""
    h = len(e) // 2
    out = []
    for x in range(4):
        s = 0
        for j in range(h):
            a0, a1, b0, b1 = (_lin(t, x, h, j) % p for t in (p0, p1, q0, q1))
            s += _lin(e, x, h, j) * ((a0 * b1 + a1 * b0 + lam * b0 % p * b1) % p)
        out.append(s % p)
    return out


def prove(field, q, seed, p_tab=None, shift=None, levels=None):
    """((N, D), proof, point, (p claim, q claim)).  levels: the sumchecks run on these ([P_0 .. P_n], [Q_0 .. Q_n]), not on the tables'
    tree -- a cheating prover"""
    p = orc.modulus(field)
    n = len(q).bit_length() - 1
    sigma = (shift or 0) % p
    P, Q = levels or tree(q, p_tab, sigma, p)
    N, D = P[0][0], Q[0][0]
    tr = _start(field, n, p_tab is not None, sigma, seed)
    tr.append(be32(N) + be32(D))
    r, cP, cQ, out = [], N, D, b""
    for j in range(n):
        h = 1 << j
        tabs = [P[j + 1][:h], P[j + 1][h:], Q[j + 1][:h], Q[j + 1][h:]]
        rho = []
        if j >= 1:
            lam = _sample(tr, field)
            tr.append(be32((cP + lam * cQ) % p))
            e = eq_table(r, p)
            for _ in range(j):
                msg = b"".join(be32(x) for x in round_evals(e, *tabs, lam, p))
                tr.append(msg)
                out += msg
                rho.append(_sample(tr, field))
                e = partial_evaluate0(e, rho[-1], p)
                tabs = [partial_evaluate0(t, rho[-1], p) for t in tabs]
        p0, p1, q0, q1 = (t[0] for t in tabs)
        msg = be32(p0) + be32(p1) + be32(q0) + be32(q1)
        tr.append(msg)
        out += msg
        tau = _sample(tr, field)
        r, cP, cQ = [tau] + rho, (p0 + tau * (p1 - p0)) % p, (q0 + tau * (q1 - q0)) % p
    assert len(out) == proof_bytes(n)
    return (N, D), out, r, (cP, (cQ - sigma) % p)


def verify(field, n, has_p, seed, total, proof, shift=None):
    """(point, (p claim, q claim)) or None"""
    p = orc.modulus(field)
    sigma = shift or 0
    N, D = total
    if not 1 <= n <= MAX_VARS or len(proof) != proof_bytes(n) or not (0 <= N < p and 0 <= D < p and 0 <= sigma < p) or D == 0:
        return None
    el = [int.from_bytes(proof[i:i + 32], "big") for i in range(0, len(proof), 32)]
    if any(x >= p for x in el):
        return None
    tr = _start(field, n, has_p, sigma, seed)
    tr.append(be32(N) + be32(D))
    r, cP, cQ, at = [], N, D, 0
    for j in range(n):
        rho, lam = [], 0
        if j >= 1:
            lam = _sample(tr, field)
            claim = (cP + lam * cQ) % p
            tr.append(be32(claim))
            for _ in range(j):
                h = el[at:at + 4]
                tr.append(proof[32 * at:32 * (at + 4)])
                at += 4
                if (h[0] + h[1]) % p != claim:
                    return None
                rho.append(_sample(tr, field))
                claim = cubic_at(h, rho[-1], p)
        p0, p1, q0, q1 = el[at:at + 4]
        tr.append(proof[32 * at:32 * (at + 4)])
        at += 4
        if j == 0:
            if N != (p0 * q1 + p1 * q0) % p or D != q0 * q1 % p:
                return None
        else:
            eq = 1
            for x, y in zip(r, rho):
                eq = eq * ((1 - x) * (1 - y) + x * y) % p
            if claim != eq * ((p0 * q1 + p1 * q0 + lam * q0 % p * q1) % p) % p:
                return None
        tau = _sample(tr, field)
        r, cP, cQ = [tau] + rho, (p0 + tau * (p1 - p0)) % p, (q0 + tau * (q1 - q0)) % p
    if not has_p and cP != 1:
        return None
    return r, (cP, (cQ - sigma) % p)


def section_offsets(n):
    """byte offsets of one element of each section of a proof of n >= 3 variables: layer 0's four values, a round evaluation of the first
    layer that has one (j = 1) and of the last, each of the last layer's four end values"""
    last = 2 * (n - 1) * n   # elements in front of layer n - 1
    end = last + 4 * (n - 1)
    out = {"l0_p0": 0, "l0_p1": 32, "l0_q0": 64, "l0_q1": 96, "round_first": 32 * 4, "round_last": 32 * (end - 1)}
    out.update({name: 32 * (end + k) for k, name in enumerate(("p0", "p1", "q0", "q1"))})
    return out


def case_inputs(case, worst_case_values):
    """(field, q, p_tab or None, shift, seed) of a shared case: tables from the worst-case limb corpus mixed with seeded random values;
    no q[i] + sigma = 0 unless the case asks for it; the shift (None for the NULL kind) by the case's hash"""
    n, v, special = case
    field = case_field(case)
    p = orc.modulus(field)
    rng = random.Random(0xF5A + hash_case(case))
    kind = case_shift_kind(case)
    shift = {"null": None, "zero": 0, "one": 1, "minus_one": p - 1, "random": rng.randrange(2, p - 1)}[kind]
    sigma = shift or 0
    worst = [x % p for x in worst_case_values(p, field, 256)]
    q = []
    while len(q) < 1 << n:
        x = rng.choice(worst) if rng.random() < 0.3 else rng.randrange(1, p)
        if (x + sigma) % p:
            q.append(x)
    p_tab = [rng.choice(worst) if rng.random() < 0.3 else rng.randrange(p) for _ in range(1 << n)] if case_has_p(case) else None
    if special == "cancel":
        q[rng.randrange(1 << n)] = (p - sigma) % p
    seed = bytes(rng.randrange(256) for _ in range(32))
    return field, q, p_tab, shift, seed


def fractional_sum(q, p_tab, shift, p):
    """sum_i p[i] / (q[i] + sigma) with modular inverses (every denominator non-zero)"""
    return sum((1 if p_tab is None else p_tab[i]) * pow((q[i] + (shift or 0)) % p, p - 2, p) for i in range(len(q))) % p


# ---- lookup multiplicities -----------------------------------------------------------------------------------------------------------
def multiplicities(table, witness):
    """(m, missing, first_missing, duplicates): m[j] = #{i : witness[i] = table[j]} if j is the lowest index holding that value, else 0;
    missing = the witness entries found nowhere in the table, first_missing the lowest such index (2^64 - 1: none); duplicates =
    len(table) - #distinct values"""
    first = {}
    for j, v in enumerate(table):
        first.setdefault(v, j)
    m = [0] * len(table)
    missing, first_missing = 0, NONE_MISSING
    for i, v in enumerate(witness):
        j = first.get(v)
        if j is None:
            missing += 1
            first_missing = min(first_missing, i)
        else:
            m[j] += 1
    return m, missing, first_missing, len(table) - len(first)


# ---- the lookup composition: two fractional sums ------------------------------------------------------------------------------------
def lookup_seeds(seed):
    """the seeds of the witness side and of the table side: keccak256(seed | 0x00), keccak256(seed | 0x01)"""
    return orc.keccak256(bytes(seed) + b"\x00"), orc.keccak256(bytes(seed) + b"\x01")


def lookup_prove(field, witness, table, alpha, seed):
    """(m, proof): every witness entry occurs in the table.  proof = ((N_f, D_f), proof_f, (N_t, D_t), proof_t): sum_i 1 / (witness[i] +
    alpha) on the first seed, sum_j m[j] / (table[j] + alpha) on the second.  m must be committed and bound by `seed` before alpha is
    drawn; the argument is sound only when the witness has fewer entries than the field's characteristic.  ValueError names first_missing"""
    m, missing, first_missing, _ = multiplicities(table, witness)
    if missing:
        raise ValueError("witness entry %d (first_missing) is not in the table; %d entries are missing" % (first_missing, missing))
    sf, st = lookup_seeds(seed)
    tot_f, proof_f, _, _ = prove(field, witness, sf, None, alpha)
    tot_t, proof_t, _, _ = prove(field, table, st, m, alpha)
    return m, (tot_f, proof_f, tot_t, proof_t)


def lookup_verify(field, n_witness, n_table, alpha, seed, proof):
    """None, or ((r_f, f_claim), (r_t, t_claim, m_claim)): what is left to check is witness(r_f) = f_claim, table(r_t) = t_claim and
    m(r_t) = m_claim"""
    p = orc.modulus(field)
    tot_f, proof_f, tot_t, proof_t = proof
    sf, st = lookup_seeds(seed)
    got_f = verify(field, n_witness, False, sf, tot_f, proof_f, alpha)
    got_t = verify(field, n_table, True, st, tot_t, proof_t, alpha)
    if got_f is None or got_t is None or tot_f[0] * tot_t[1] % p != tot_t[0] * tot_f[1] % p:
        return None
    return (got_f[0], got_f[1][1]), (got_t[0], got_t[1][1], got_t[1][0])
