"""The definition of the library's wiring (copy-constraint) permutation argument (zk_mle_perm_fingerprint, zk_perm_prove,
zk_perm_verify_host, zk_perm_proof_bytes; the reference has nothing like it, so this file is the definition), built on the grand-product
argument's definition (tests/gprod_ref.py, imported and left as it is), and the cases the host and GPU tests share.  Everything is
bytes: no tolerance.

  parameters  the field; k witness columns w_c and k permutation columns sigma_c (1 <= k <= 16), all of n >= 1 variables (variable 0 =
              the index's top bit); challenges beta, gamma; a 32-byte seed.  Cell (c, i) has the label c 2^n + i, and sigma_c[i] is the
              label of the cell (c, i) is wired to, as a field element
  sizes       K = 2^kappa the next power of two >= k, N = n + kappa + 1 <= 40
  fingerprint F of N variables, the side bit the LOWEST index bit: for v = c 2^n + i, c < k: F[2v] = w_c[i] + beta v + gamma (identity
              side), F[2v + 1] = w_c[i] + beta sigma_c[i] + gamma (sigma side); for k <= c < K both are 1
  products    gprod_ref's tree multiplies the top index bit away first, so level 1 is (identity side's product, sigma side's product)
  proof       gprod_ref.prove(F, NULL shift, seed') with seed' = Keccak-256(seed | be64(field id) be64(n) be64(k) | be32(beta) |
              be32(gamma)), then w_0(r_lo) .. w_{k-1}(r_lo), sigma_0(r_lo) .. sigma_{k-1}(r_lo): 2 N^2 + 2 k elements of 32 bytes,
              big-endian canonical.  No product is sent
  verify      a, b = the first two elements; a == b; gprod_ref.verify with the product a b; its point (r_hi: kappa, r_lo: n, r_s: 1) and
              claim; accept iff claim = sum_{c<k} eq(r_hi, c) (vw_c + beta ((1 - r_s)(c 2^n + sum_b r_lo[b] 2^(n-1-b)) + r_s vs_c) + gamma)
              + sum_{k<=c<K} eq(r_hi, c).  The output is r_lo and the 2 k claims w_c(r_lo) = vw_c, sigma_c(r_lo) = vs_c that the caller
              checks (one batch opening).  Nothing is sized by 2^n
  binding     the tables are not absorbed: the seed must bind the commitments of w and sigma, and beta, gamma must be drawn after that.
              That sigma is a permutation of the labels is the circuit's preprocessing to guarantee.  The prover does not check the
              statement: on broken wiring it makes these bytes and the verifier rejects"""
import random

import gprod_ref as gp
from oracle import binding as orc

MAX_COLS = 16
MAX_VARS = gp.MAX_VARS

# (n, k, variant, broken): N <= 10 runs on the LDS stage alone; N = 11, 12, 13, 14 is one, two, three and four levels above it (the fused
# route, ZK_PERM_FUSE=1: k_perm_tree<1>, <2>, <2> and a k_ptree<1>, <2> and a k_ptree<2>); kappa = 0 .. 4; the fused levels all column
# bits (k = 5, 8, 9, 16), straddling column and row bits (k = 2 at A = 2), all row bits (k = 1); padding columns (k = 3, 5, 9); broken =
# 1: one copy is violated
HOST_CASES = ((1, 1, 0, 0), (2, 1, 0, 0), (3, 2, 0, 0), (2, 3, 0, 0), (3, 5, 0, 0), (4, 8, 0, 0), (6, 3, 0, 0), (3, 16, 0, 0), (2, 9, 0, 0),
              (3, 2, 1, 1), (4, 5, 1, 1), (1, 1, 1, 1))
GPU_SMALL_CASES = ((1, 1, 0, 0), (3, 2, 0, 0), (2, 3, 0, 0), (4, 5, 0, 0), (5, 8, 0, 0), (4, 16, 0, 0), (5, 3, 1, 1))
GPU_FUSED_CASES = ((6, 16, 0, 0), (8, 5, 0, 0), (10, 3, 0, 0), (11, 2, 0, 0), (12, 1, 0, 0), (9, 8, 0, 0), (9, 9, 0, 0))
GPU_CASES = GPU_SMALL_CASES + GPU_FUSED_CASES


def be32(v):
    return int(v).to_bytes(32, "big")


def kappa(k):
    return (k - 1).bit_length()


def total_vars(n, k):
    return n + kappa(k) + 1


def proof_bytes(n, k):
    N = total_vars(n, k)
    return 32 * (2 * N * N + 2 * k)


def case_key(case):
    return "n%d_k%d_v%d_b%d" % case


def case_field(case):
    return (case[0] + 2 * case[1] + case[2]) % 3


def seed_prime(field, n, k, beta, gamma, seed):
    assert len(seed) == 32
    return orc.keccak256(bytes(seed) + b"".join(int(x).to_bytes(8, "big") for x in (field, n, k)) + be32(beta) + be32(gamma))


def fingerprint(field, w, sigma, beta, gamma):
    p = orc.modulus(field)
    k, rows = len(w), len(w[0])
    out = []
    for c in range(1 << kappa(k)):
        for i in range(rows):
            if c < k:
                v = c * rows + i
                out += [(w[c][i] + beta * v + gamma) % p, (w[c][i] + beta * sigma[c][i] + gamma) % p]
            else:
                out += [1, 1]
    return out


def prove(field, w, sigma, beta, gamma, seed):
    """(proof, point, claims): point = r_lo, claims = [w_c(r_lo)] + [sigma_c(r_lo)]"""
    p = orc.modulus(field)
    k, n = len(w), len(w[0]).bit_length() - 1
    assert len(sigma) == k and 1 <= k <= MAX_COLS and n >= 1
    _, head, r, _ = gp.prove(field, fingerprint(field, w, sigma, beta, gamma), seed_prime(field, n, k, beta, gamma, seed))
    r_lo = r[kappa(k):kappa(k) + n]
    claims = [gp.evaluate(t, r_lo, p) for t in list(w) + list(sigma)]
    proof = head + b"".join(be32(x) for x in claims)
    assert len(proof) == proof_bytes(n, k)
    return proof, r_lo, claims


def closing_value(p, n, k, beta, gamma, point, claims, drop_padding=False):
    """F(point) from the 2 k end values: what the grand product's claim must equal.  drop_padding: without the padding columns' ones
    (a wrong verifier, for the tests)"""
    kp = kappa(k)
    r_hi, r_lo, r_s = point[:kp], point[kp:kp + n], point[kp + n]
    ident = sum(r_lo[b] << (n - 1 - b) for b in range(n))
    eq_hi = gp.eq_table(r_hi, p)
    total = 0
    for c in range(1 << kp):
        if c < k:
            label = (1 - r_s) * ((c << n) + ident) + r_s * claims[k + c]
            total += eq_hi[c] * (claims[c] + beta * label + gamma)
        elif not drop_padding:
            total += eq_hi[c]
    return total % p


def verify(field, n, k, beta, gamma, seed, proof, drop_padding=False):
    """(point, claims) or None"""
    p = orc.modulus(field)
    if not 1 <= k <= MAX_COLS or n < 1 or total_vars(n, k) > MAX_VARS or len(proof) != proof_bytes(n, k):
        return None
    if not (0 <= beta < p and 0 <= gamma < p):
        return None
    N = total_vars(n, k)
    head, tail = proof[:gp.proof_bytes(N)], proof[gp.proof_bytes(N):]
    claims = [int.from_bytes(tail[i:i + 32], "big") for i in range(0, len(tail), 32)]
    a, b = int.from_bytes(head[:32], "big"), int.from_bytes(head[32:64], "big")
    if any(x >= p for x in claims) or a >= p or b >= p or a != b:
        return None
    got = gp.verify(field, N, seed_prime(field, n, k, beta, gamma, seed), a * b % p, head)
    if got is None:
        return None
    point, claim = got
    if claim != closing_value(p, n, k, beta, gamma, point, claims, drop_padding):
        return None
    return point[kappa(k):kappa(k) + n], claims


def wiring_sigma(classes):
    """classes: k rows of 2^n copy-class ids -> k rows of labels: every class's cells, in label order, wired in one cycle"""
    rows = len(classes[0])
    cells = {}
    for c, col in enumerate(classes):
        for i, cid in enumerate(col):
            cells.setdefault(int(cid), []).append(c * rows + i)
    sigma = [[0] * rows for _ in classes]
    for members in cells.values():
        for j, v in enumerate(members):
            nxt = members[(j + 1) % len(members)]
            sigma[v // rows][v % rows] = nxt
    return sigma


def section_offsets(n, k):
    """byte offsets of one element of each section: the grand product's (gprod_ref.section_offsets, N >= 3), the first and last w value,
    the first and last sigma value"""
    N = total_vars(n, k)
    out = dict(gp.section_offsets(N))
    base = gp.proof_bytes(N)
    out.update({"w_first": base, "w_last": base + 32 * (k - 1), "s_first": base + 32 * k, "s_last": base + 32 * (2 * k - 1)})
    return out


def case_inputs(case, worst_case_values):
    """(field, w, sigma, beta, gamma, seed) of a shared case: random copy classes (about two cells per class, some single), one value
    per class from the worst-case limb corpus mixed with seeded random values; broken: one cell of a class of two or more is changed"""
    n, k, variant, broken = case
    field = case_field(case)
    p = orc.modulus(field)
    rng = random.Random(0x9E7 + 1000 * n + 10 * k + variant)
    rows = 1 << n
    n_classes = max(1, (k * rows) // 2)
    classes = [[rng.randrange(n_classes) for _ in range(rows)] for _ in range(k)]
    classes[0][0] = classes[k - 1][rows - 1] = 0   # a class of two cells at least (one cell when k 2^n = 1 ... n >= 1: never)
    worst = worst_case_values(p, field, 256)
    value = {}
    w = [[value.setdefault(cid, rng.choice(worst) % p if rng.random() < 0.3 else rng.randrange(p)) for cid in col] for col in classes]
    sigma = wiring_sigma(classes)
    if broken:
        w[0][0] = (w[0][0] + 1) % p
    beta, gamma = rng.randrange(1, p), rng.randrange(1, p)
    seed = bytes(rng.randrange(256) for _ in range(32))
    return field, w, sigma, beta, gamma, seed
