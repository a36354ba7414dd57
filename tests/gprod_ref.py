"""The definition of the library's grand-product argument (zk_mle_product_tree, zk_gprod_prove, zk_gprod_verify_host,
zk_gprod_proof_bytes; the reference has nothing like it, so this file is the definition): a binary product tree whose layers are tied
together by one degree-3 sumcheck each, all on one transcript, in plain Python integers over the C oracle's transcript, and the cases the
host and GPU tests share.  Everything is bytes: no tolerance.

  parameters  the field, a table t of 2^n values (n >= 1; variable 0 = the index's top bit), a shift sigma (None = 0, the same bytes as an
              explicit 0), a 32-byte seed
  tree        V_n[i] = t[i] + sigma; V_j[i] = V_{j+1}[i] V_{j+1}[i + 2^j] for i < 2^j, j = n-1 .. 0: the low half times the high half, so
              the split is variable 0 of V_{j+1}; P = V_0[0].  product_tree() is the heap the device call returns: out[0] = 1,
              out[2^j + i] = V_j[i] for j < n
  transcript  orc.Transcript(); the seed; be64(field id), be64(n); be32(sigma)
  layers      j = 0 .. n-1, each a claim c_j = V_j(r_j) at a point r_j of j elements; r_0 = (), c_0 = P.  Layer j: absorb be32(c_j); for
              j >= 1 the sumcheck of sum_x E(x) A(x) B(x) over {0,1}^j with E = eq(., r_j), A = V_{j+1}[0 : 2^j], B = V_{j+1}[2^j : 2^(j+1)],
              exactly prove_partial on a product of three tables of degree 3 continuing the transcript: round i sends h(X) = sum_x'
              E(X,x') A(X,x') B(X,x') at X = 0, 1, 2, 3 (absorbed as 4 x be32), rho_i = sample_field_element, all three tables folded with
              partial_evaluate(0, [rho_i]).  Then a = V_{j+1}(0, rho), b = V_{j+1}(1, rho) (at j = 0: V_1[0], V_1[1]), absorbed as 2 x be32;
              tau_j = sample_field_element; r_{j+1} = (tau_j, rho_0 .. rho_{j-1}); c_{j+1} = a + tau_j (b - a)
  proof       per layer the 4 j round evaluations, then a, b: 2 n^2 elements of 32 bytes, big-endian canonical.  P is the public claim,
              beside the proof
  verify      exact length; every element and P canonical (else the verdict is False, not an error); the transcript rebuilt; per round
              h(0) + h(1) = claim, the new claim h(rho_i) by the cubic through 0..3; at a layer's end claim = eq(r_j, rho) a b (layer 0:
              a b = P).  The output is the point r_n and the value c_n - sigma: the claim t(r_n) = c_n - sigma that the caller checks
  binding     the argument does not absorb the table (prove_partial does not either): the seed must bind it, e.g. a commitment's root"""
import random

from oracle import binding as orc

MAX_VARS = 40
# ---- the tree kernels' shape (zk_amd/csrc/gprod_kernels.cuh, gprod.hip; tests/test_gprod_host.py matches the constants named here) ------
# Levels above 2^LDS_VARS elements are taken down FUSE levels per launch (k_ptree<A>, A = min(FUSE, what is left), from the top), then one
# workgroup finishes levels LDS_VARS .. 0 out of LDS (k_ptree_lds).  A fused launch has one thread per element of its lowest level on a
# grid capped at MAX_BLOCKS_STREAM workgroups, and a wave loops over runs of 64 elements.
LDS_VARS = 10                                   # kPtreeLdsVars
FUSE_MAX, FUSE_DEFAULT = 3, 3                   # kPtreeMaxFuse, kPtreeFuseDefault
THREADS, MAX_BLOCKS_STREAM = 256, 16384         # kBlock, kMaxGridStream


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


# the smallest n at which the capped grid's loop takes a second trip, per switch setting: {1: 24, 2: 25, 3: 26}.  On the default route
# (FUSE_DEFAULT = 3) that is 2^26 elements -- not below 2^25, so there is no default-route table to test; one level per launch loops
# from 2^24 on, which the GPU test runs against the C oracle
SECOND_TRIP_VARS = {f: next(n for n in range(1, MAX_VARS + 1) if trips(n, f) == 2) for f in range(1, FUSE_MAX + 1)}

SHIFT_KINDS = ("null", "zero", "one", "minus_one", "random")
# (n, variant, special): n = 1..8 twice; special "zero" = the table holds a zero, "cancel" = t[i] + sigma = 0 for one i (P = 0 either way)
CASES = tuple((n, v, "") for n in range(1, 9) for v in (0, 1)) + ((5, 2, "zero"), (6, 2, "cancel"))
# what the GPU test adds: 1, 2, 3 and 4 levels above the LDS stage (one fused launch of each arity, then two launches), one per field
GPU_EXTRA_CASES = tuple((LDS_VARS + k, 3, "") for k in (1, 2, 3, 4))
GPU_CASES = CASES + GPU_EXTRA_CASES
# zk_mle_product_tree alone against Python integers: every size up to two past the LDS stage
TREE_VARS = tuple(range(1, LDS_VARS + 3))


def be32(v):
    return int(v).to_bytes(32, "big")


def hash_case(case):
    n, v, special = case
    return (2 * n + v) * 7 + 3 + len(special)


def case_field(case):
    """spread by the hash; the GPU extras (variant 3) take the three fields in turn"""
    return case[0] % 3 if case[1] == 3 else (hash_case(case) // 5) % 3


def case_shift_kind(case):
    return "random" if case[2] == "cancel" else SHIFT_KINDS[hash_case(case) % 5]


def proof_bytes(n):
    return 64 * n * n


def eq_table(z, p):
    """eq(., z) in hypercube order: variable 0 = the index's top bit"""
    out = [1]
    for zj in z:
        out = [e * w % p for e in out for w in ((1 - zj) % p, zj % p)]
    return out


def partial_evaluate0(t, r, p):
    """partial_evaluate(0, [r]): the top index bit"""
    h = len(t) // 2
    return [(t[j] + r * (t[j + h] - t[j])) % p for j in range(h)]


def evaluate(t, z, p):
    for zj in z:
        t = partial_evaluate0(t, zj, p)
    return t[0]


def tree(table, shift, p):
    """[V_0, .., V_n]"""
    n = len(table).bit_length() - 1
    assert len(table) == 1 << n and n >= 1
    levels = [[(x + (shift or 0)) % p for x in table]]
    for j in range(n - 1, -1, -1):
        up = levels[0]
        levels.insert(0, [up[i] * up[i + (1 << j)] % p for i in range(1 << j)])
    return levels


def product_tree(table, shift, p):
    """the heap zk_mle_product_tree returns: 2^n elements"""
    levels = tree(table, shift, p)
    return [1] + [x for level in levels[:-1] for x in level]


def cubic_at(h, x, p):
    """the cubic through (0, h[0]) .. (3, h[3]) at x"""
    inv6, inv2 = pow(6, p - 2, p), pow(2, p - 2, p)
    l0 = -(x - 1) * (x - 2) * (x - 3) * inv6
    l1 = x * (x - 2) * (x - 3) * inv2
    l2 = -x * (x - 1) * (x - 3) * inv2
    l3 = x * (x - 1) * (x - 2) * inv6
    return (h[0] * l0 + h[1] * l1 + h[2] * l2 + h[3] * l3) % p


def _start(field, n, shift, seed):
    assert len(seed) == 32
    tr = orc.Transcript()
    tr.append(bytes(seed))
    tr.append(int(field).to_bytes(8, "big") + int(n).to_bytes(8, "big"))
    tr.append(be32(shift or 0))
    return tr


def _sample(tr, field):
    return orc.to_int(field, tr.sample_field_element(field))


def round_evals(e, a, b, p):
    """h(X) = sum_x' E(X,x') A(X,x') B(X,x') at X = 0, 1, 2, 3"""
    h = len(e) // 2
    out = []
    for x in range(4):
        out.append(sum((e[j] + x * (e[j + h] - e[j])) * (a[j] + x * (a[j + h] - a[j])) % p * (b[j] + x * (b[j + h] - b[j])) for j in range(h)) % p)
    return out


def prove(field, table, seed, shift=None, levels=None):
    """(P, proof, point, claim).  levels: the sumchecks run on these [V_0 .. V_n], not on the table's tree -- a cheating prover"""
    p = orc.modulus(field)
    n = len(table).bit_length() - 1
    sigma = (shift or 0) % p
    levels = levels or tree(table, sigma, p)
    product = levels[0][0]
    tr = _start(field, n, sigma, seed)
    r, c, out = [], product, b""
    for j in range(n):
        tr.append(be32(c))
        up = levels[j + 1]
        e, a, b, rho = eq_table(r, p), up[:1 << j], up[1 << j:], []
        for _ in range(j):
            h = b"".join(be32(x) for x in round_evals(e, a, b, p))
            tr.append(h)
            out += h
            rho.append(_sample(tr, field))
            e, a, b = (partial_evaluate0(x, rho[-1], p) for x in (e, a, b))
        ab = be32(a[0]) + be32(b[0])
        tr.append(ab)
        out += ab
        tau = _sample(tr, field)
        r, c = [tau] + rho, (a[0] + tau * (b[0] - a[0])) % p
    assert len(out) == proof_bytes(n)
    return product, out, r, (c - sigma) % p


def verify(field, n, seed, product, proof, shift=None):
    """(point, claim) or None"""
    p = orc.modulus(field)
    sigma = shift or 0
    if not 1 <= n <= MAX_VARS or len(proof) != proof_bytes(n) or not 0 <= product < p or not 0 <= sigma < p:
        return None
    el = [int.from_bytes(proof[i:i + 32], "big") for i in range(0, len(proof), 32)]
    if any(x >= p for x in el):
        return None
    tr = _start(field, n, sigma, seed)
    r, c, at = [], product, 0
    for j in range(n):
        tr.append(be32(c))
        claim, rho = c, []
        for i in range(j):
            h = el[at:at + 4]
            tr.append(proof[32 * at:32 * (at + 4)])
            at += 4
            if (h[0] + h[1]) % p != claim:
                return None
            rho.append(_sample(tr, field))
            claim = cubic_at(h, rho[-1], p)
        a, b = el[at:at + 2]
        tr.append(proof[32 * at:32 * (at + 2)])
        at += 2
        eq = 1
        for x, y in zip(r, rho):
            eq = eq * ((1 - x) * (1 - y) + x * y) % p
        if claim != eq * a % p * b % p:
            return None
        tau = _sample(tr, field)
        r, c = [tau] + rho, (a + tau * (b - a)) % p
    return r, (c - sigma) % p


def section_offsets(n):
    """byte offsets of one element of each section of a proof of n >= 3 variables: layer 0's pair, a round evaluation of the first layer
    that has one (j = 1) and of the last, an a and a b"""
    last = 2 * (n - 1) * (n - 1)   # elements in front of layer n - 1
    return {"pair0": 0, "round_first": 32 * 2, "round_last": 32 * (last + 4 * (n - 1) - 1), "a": 32 * (last + 4 * (n - 1)),
            "b": 32 * (last + 4 * (n - 1) + 1)}


def case_inputs(case, worst_case_values):
    """(field, table, shift, seed) of a shared case: the table from the worst-case limb corpus mixed with seeded random values, no entry
    0 or -sigma unless the case asks for one; the shift (None for the NULL kind) by the case's hash"""
    n, v, special = case
    field = case_field(case)
    p = orc.modulus(field)
    rng = random.Random(0x69D + hash_case(case))
    kind = case_shift_kind(case)
    shift = {"null": None, "zero": 0, "one": 1, "minus_one": p - 1, "random": rng.randrange(2, p - 1)}[kind]
    sigma = shift or 0
    worst = [x for x in worst_case_values(p, field, 256) if x % p and (x + sigma) % p]
    table = []
    while len(table) < 1 << n:
        x = rng.choice(worst) % p if rng.random() < 0.3 else rng.randrange(1, p)
        if (x + sigma) % p:
            table.append(x)
    if special == "zero":
        table[rng.randrange(1 << n)] = 0
    if special == "cancel":
        table[rng.randrange(1 << n)] = (p - sigma) % p
    seed = bytes(rng.randrange(256) for _ in range(32))
    return field, table, shift, seed
