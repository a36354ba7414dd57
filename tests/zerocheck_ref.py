"""The definition of the library's zerocheck argument (zk_gate_create, zk_zerocheck_prove, zk_zerocheck_verify_host,
zk_zerocheck_proof_bytes, zk_mle_gate_sums; the reference has nothing like it, so this file is the definition): a custom gate holds on
every row of k columns, in plain Python integers over the C oracle's transcript, and the cases the host and GPU tests share.  Everything
is bytes: no tolerance.

  gate        G(x_0 .. x_{k-1}) = sum_{i < T} c_i prod_{f in term i} x_f: here (k, [(c_i, (f, ..)), ..]).  A term is a list of column
              indices; a repeat is a power, the empty term a constant; a column may appear in any number of terms, or in none.  The degree
              d is the longest term.  Limits: 1 <= k <= 16, 1 <= T <= 32, 1 <= d <= 6, at most 64 factor mentions in all
  statement   G(t_0[i], .., t_{k-1}[i]) = 0 for every i < 2^n (n >= 1; variable 0 = the index's top bit)
  transcript  orc.Transcript(); the seed; be64(field id), be64(n), be64(k), be64(T); per term be32(c_i) canonical, be64(length), be64 per
              factor.  Then tau_0 .. tau_{n-1} by sample_field_element
  rounds      j = 0 .. n-1, m = n-1-j: the eq-factored message
                  g_j(X) = sum_{x' < 2^m} eq(x', (tau_{j+1} ..)) G(T_j(X, x')),  X = 0 .. d
              with T_j(X, x') = T_j[x'] + X (T_j[2^m + x'] - T_j[x']) per column (the factors eq(tau_{<j}, rho_{<j}) and eq(tau_j, X) are
              not in it); absorb g_j(0) .. g_j(d) as be32; rho_j = sample_field_element; T_{j+1} = partial_evaluate(0, [rho_j]) of every
              column.  After the last round the k values v_c = t_c(rho) are absorbed
  proof       n (d + 1) + k elements of 32 bytes, big-endian canonical
  verify      exact length; every element canonical (else the verdict is False, not an error); e_0 = 0; per round
              (1 - tau_j) g_j(0) + tau_j g_j(1) = e_j, then e_{j+1} = g_j(rho_j) by interpolation on 0 .. d; at the end G(v) = e_n.  The
              output is the point rho and the k claims v: t_c(rho) = v_c is what the caller checks, e.g. with one batch opening
  soundness   multiply round j's message by s_j eq(tau_j, X), s_j = prod_{i<j} eq(tau_i, rho_i): an accepting transcript becomes an
              accepting transcript of the plain degree-(d + 1) sumcheck of sum_x eq(tau, x) G(t(x)) = 0
  binding     the argument does not absorb the tables (prove_partial does not either): the seed must bind them, e.g. the root of their
              batch commitment
The prover does not check the statement: on tables that violate the gate it makes these bytes, and verify rejects them."""
import random

from oracle import binding as orc

MAX_VARS = 40
MAX_COLS, MAX_TERMS, MAX_DEGREE, MAX_MENTIONS = 16, 32, 6, 64

# ---- the round kernel's schedule (zk_amd/csrc/zerocheck_kernels.cuh, zerocheck.hip ZcSide::round) ---------------------------------------
# Round j sums over 2^m x', m = n - 1 - j.  m < RUN_MIN_BITS: one workgroup, one x' per thread.  Else a wave takes runs of 2^S x' that
# share one Hi entry, S = min(L, max(6, m - RUNS_TARGET_LOG)), L = min(m, LO_BITS): Lo (2^L entries) is the whole weight up to m = LO_BITS.
# The grid is capped at MAX_BLOCKS workgroups of 256 threads (k <= WIDE_COLS) or 128 (above): past that a wave loops over runs.
LO_BITS, RUN_MIN_BITS, RUNS_TARGET_LOG, MAX_BLOCKS, WIDE_COLS = 9, 6, 11, 2048, 8


def run_log(m):
    """S of the launch over 2^m x'; None below the run kernel"""
    if m < RUN_MIN_BITS:
        return None
    fit = m - RUNS_TARGET_LOG if m > RUNS_TARGET_LOG + RUN_MIN_BITS else RUN_MIN_BITS
    return min(fit, min(m, LO_BITS))


def runs_per_wave(m, k):
    s = run_log(m)
    if s is None:
        return 0
    waves = (256 if k <= WIDE_COLS else 128) // 64
    n_runs = 1 << (m - s)
    blocks = min(-(-n_runs // waves), MAX_BLOCKS)
    return -(-n_runs // (blocks * waves))


# the smallest n (round 0: m = n - 1) at which a run grows past 64 elements: 19 -- the proof at 2^20 covers it (S = 8 in round 0, 7 in
# round 1).  The smallest n at which a wave takes a second run: 24 with 256 threads, 23 with 128 (k > 8) -- tables of 512 and 256 MiB
# per column, out of a test's reach; tools/zerocheck_bench.py runs n = 24.
RUN_GROWS_VARS = next(n for n in range(1, MAX_VARS + 1) if (run_log(n - 1) or 0) > 6)
SECOND_RUN_VARS = {k: next(n for n in range(1, MAX_VARS + 1) if runs_per_wave(n - 1, k) == 2) for k in (8, 16)}


# ---- the gates -----------------------------------------------------------------------------------------------------------------------
def _limits_gate():
    """every limit at once: k = 16, T = 32, 64 mentions, d = 6; column 15 is mentioned once (case_inputs solves for it)"""
    rng = random.Random(0x2C0)
    lens = [6, 1] + [2] * 27 + [1] * 3
    terms = []
    for i, ln in enumerate(lens):
        cols = (15,) if i == 1 else tuple(rng.randrange(15) for _ in range(ln))
        coeff = (1, -1, rng.randrange(1 << 250))[i % 3]
        terms.append((coeff, cols))
    return 16, terms


# columns of the Plonk gate: a, b, c, qL, qR, qM, qO, qC
GATES = {
    "x0": (1, [(1, (0,))]),
    "mul": (3, [(1, (0, 1)), (-1, (2,))]),
    "plonk": (8, [(1, (3, 0)), (1, (4, 1)), (1, (5, 0, 1)), (1, (6, 2)), (1, (7,))]),
    "deg6": (3, [(1, (2, 0, 0, 0, 0, 0)), (-1, (2, 1))]),
    "limits": _limits_gate(),
    "const": (4, [(3, ()), (0, (0, 1)), (2, (2,)), (1 << 200, (1, 1))]),   # a constant, a zero coefficient, column 3 unmentioned
}
GATE_NAMES = tuple(GATES)
assert sum(len(c) for _, c in GATES["limits"][1]) == MAX_MENTIONS and len(GATES["limits"][1]) == MAX_TERMS


def gate_degree(gate):
    return max(len(cols) for _, cols in gate[1])


def gate_mod(gate, p):
    return gate[0], [(c % p, tuple(cols)) for c, cols in gate[1]]


def gate_eval(terms, vals, p):
    acc = 0
    for c, cols in terms:
        for f in cols:
            c = c * vals[f] % p
        acc += c
    return acc % p


# (n, gate, variant): every n = 1 .. 13 with two gates each, variant 0 = a satisfying instance, 1 = the worst-case limb corpus (which
# does not satisfy the gate; the comparison is byte parity all the same).  The limits gate stays at n <= 10: the definition is Python.
def _cases():
    out = []
    cheap = [g for g in GATE_NAMES if g != "limits"]
    for n in range(1, 14):
        names = [cheap[n % 5], cheap[(n + 2) % 5]]
        if n in (1, 4, 7, 10):
            names[1] = "limits"
        out += [(n, names[0], 0), (n, names[1], 1)]
    return tuple(out)


CASES = _cases() + ((6, "plonk", 1), (11, "plonk", 0), (10, "deg6", 1), (2, "limits", 0))


def be32(v):
    return int(v).to_bytes(32, "big")


def hash_case(case):
    return (case[0] * 6 + GATE_NAMES.index(case[1])) * 2 + case[2]


def case_field(case):
    return hash_case(case) % 3


def case_key(case):
    return "n%d_%s_v%d" % case


def proof_bytes(gate, n):
    return 32 * (n * (gate_degree(gate) + 1) + gate[0])


def eq_table(z, p):
    """eq(., z) in hypercube order: variable 0 = the index's top bit"""
    out = [1]
    for zj in z:
        out = [e * w % p for e in out for w in ((1 - zj) % p, zj % p)]
    return out


def partial_evaluate0(t, r, p):
    h = len(t) // 2
    return [(t[j] + r * (t[j + h] - t[j])) % p for j in range(h)]


def evaluate(t, z, p):
    for zj in z:
        t = partial_evaluate0(t, zj, p)
    return t[0]


def round_message(terms, d, tables, weights, p):
    """g(X) = sum_x' weights[x'] G(T(X, x')), X = 0 .. d"""
    half = len(tables[0]) // 2
    g = [0] * (d + 1)
    for x in range(half):
        lo = [t[x] for t in tables]
        df = [t[x + half] - t[x] for t in tables]
        w = weights[x]
        for big_x in range(d + 1):
            g[big_x] += w * gate_eval(terms, [a + big_x * b for a, b in zip(lo, df)], p)
    return [v % p for v in g]


def gate_sums(field, gate, tables, tail):
    """zk_mle_gate_sums: the round message of the tables as they are against eq(., tail)"""
    p = orc.modulus(field)
    k, terms = gate_mod(gate, p)
    return round_message(terms, gate_degree(gate), tables, eq_table(tail, p), p)


def lagrange_at(g, x, p):
    """the polynomial through (0, g[0]) .. (d, g[d]) at x"""
    acc = 0
    for t in range(len(g)):
        num, den = 1, 1
        for u in range(len(g)):
            if u != t:
                num = num * (x - u) % p
                den = den * (t - u) % p
        acc += g[t] * num % p * pow(den, p - 2, p)
    return acc % p


def _start(field, gate, n, seed, p):
    assert len(seed) == 32
    k, terms = gate_mod(gate, p)
    tr = orc.Transcript()
    tr.append(bytes(seed))
    tr.append(b"".join(int(v).to_bytes(8, "big") for v in (field, n, k, len(terms))))
    for c, cols in terms:
        tr.append(be32(c) + len(cols).to_bytes(8, "big") + b"".join(int(f).to_bytes(8, "big") for f in cols))
    return tr


def _sample(tr, field):
    return orc.to_int(field, tr.sample_field_element(field))


def prove(field, gate, tables, seed):
    """(proof, point, claims)"""
    p = orc.modulus(field)
    k, terms = gate_mod(gate, p)
    d = gate_degree(gate)
    n = len(tables[0]).bit_length() - 1
    assert len(tables) == k and n >= 1 and all(len(t) == 1 << n for t in tables)
    tr = _start(field, gate, n, seed, p)
    tau = [_sample(tr, field) for _ in range(n)]
    cur, rho, out = [list(t) for t in tables], [], b""
    for j in range(n):
        msg = b"".join(be32(v) for v in round_message(terms, d, cur, eq_table(tau[j + 1:], p), p))
        tr.append(msg)
        out += msg
        rho.append(_sample(tr, field))
        cur = [partial_evaluate0(t, rho[-1], p) for t in cur]
    claims = [t[0] for t in cur]
    fin = b"".join(be32(v) for v in claims)
    tr.append(fin)
    out += fin
    assert len(out) == proof_bytes(gate, n)
    return out, rho, claims


def verify(field, gate, n, seed, proof):
    """(point, claims) or None"""
    p = orc.modulus(field)
    k, terms = gate_mod(gate, p)
    d = gate_degree(gate)
    if not 1 <= n <= MAX_VARS or len(proof) != proof_bytes(gate, n):
        return None
    el = [int.from_bytes(proof[i:i + 32], "big") for i in range(0, len(proof), 32)]
    if any(x >= p for x in el):
        return None
    tr = _start(field, gate, n, seed, p)
    tau = [_sample(tr, field) for _ in range(n)]
    e, rho = 0, []
    for j in range(n):
        g = el[j * (d + 1):(j + 1) * (d + 1)]
        if ((1 - tau[j]) * g[0] + tau[j] * g[1]) % p != e:
            return None
        tr.append(proof[32 * j * (d + 1):32 * (j + 1) * (d + 1)])
        rho.append(_sample(tr, field))
        e = lagrange_at(g, rho[-1], p)
    v = el[n * (d + 1):]
    if gate_eval(terms, v, p) != e:
        return None
    return rho, v


def section_offsets(gate, n):
    """byte offsets of one element per position class: a g_j(0), a g_j(d), a final value (of a column that a term with a non-zero
    coefficient mentions: the value of a column the gate ignores is not checked by the argument)"""
    d = gate_degree(gate)
    col = next(f for c, cols in gate[1] if c for f in cols)
    return {"g0": 32 * ((n // 2) * (d + 1)), "gd": 32 * ((n - 1) * (d + 1) + d), "final": 32 * (n * (d + 1) + col)}


def satisfying_tables(gate, n, p, rng):
    """k columns of 2^n values with G = 0 on every row: random values, and the column that is mentioned once (in a term with a
    non-zero coefficient) solved for"""
    k, terms = gate_mod(gate, p)
    mentions = [f for _, cols in terms for f in cols]
    solve, at = next((f, i) for i, (c, cols) in enumerate(terms) for f in cols if mentions.count(f) == 1 and c)
    rest_terms = terms[:at] + terms[at + 1:]
    c_at, others = terms[at][0], [f for f in terms[at][1] if f != solve]
    rows = []
    while len(rows) < 1 << n:
        vals = [rng.randrange(p) for _ in range(k)]
        coeff = gate_eval([(c_at, tuple(others))], vals, p)
        if coeff == 0:
            continue
        vals[solve] = -gate_eval(rest_terms, vals, p) * pow(coeff, p - 2, p) % p
        rows.append(vals)
    return [[row[c] for row in rows] for c in range(k)]


def case_inputs(case, worst_case_values):
    """(field, gate, tables, seed) of a shared case"""
    n, name, variant = case
    field, gate = case_field(case), GATES[name]
    p = orc.modulus(field)
    rng = random.Random(0x2E0 + hash_case(case))
    if variant == 0:
        tables = satisfying_tables(gate, n, p, rng)
        assert all(gate_eval(gate_mod(gate, p)[1], [t[i] for t in tables], p) == 0 for i in range(1 << n))
    else:
        worst = [x % p for x in worst_case_values(p, field, 256)]
        tables = [[rng.choice(worst) if rng.random() < 0.5 else rng.randrange(p) for _ in range(1 << n)] for _ in range(gate[0])]
    seed = bytes(rng.randrange(256) for _ in range(32))
    return field, gate, tables, seed
