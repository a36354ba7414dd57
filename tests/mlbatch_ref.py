"""The definition of the library's batch multilinear commitment (zk_mlbatch_commit, zk_mlbatch_open, zk_mlbatch_verify_host,
zk_mlbatch_proof_bytes, zk_mle_lincomb, zk_mle_eq_sums_many; the reference has nothing like it, so this file is the definition): k tables
of one size under one Merkle tree, opened at m points by ONE BaseFold opening (tests/mlpcs_ref.py) of a random linear combination, in
plain Python integers over tests/mlpcs_ref.py, tests/fri_ref.py, tests/merkle_ref.py, tests/cmle_ref.py and the C oracle's transcript, and
the cases the host and GPU tests share.  Everything is bytes: no tolerance.

  parameters  the field; k tables t_0 .. t_{k-1} (1 <= k <= 256) of 2^n values each, the same n >= 1 for all (tables of another size go
              into another commitment); b, f, Q and the shift s as in mlpcs_ref; m points z_0 .. z_{m-1} (1 <= m <= 16) of n elements
              each, repeated points allowed; R = n - f rounds
  commit      F_0^c = fri_ref.lde(cmle_ref.interpolate_fast(t_c), n + b, s) for every c; one Merkle tree over the 2k column views of
              M_0 = 2^(n+b-1) rows: column 2c = F_0^c[0:M_0], column 2c + 1 = F_0^c[M_0:2 M_0]; the commitment is its root (k = 1:
              mlpcs_ref.commit's root)
  open        v[j][c] = t_c(z_j), the full m x k matrix.  Transcript: seed; be64 of field id, n, b, f, Q, k, m; be32(s); root; every z_j
              (be32 per element, j-major); every v[j][c] (j-major); lambda = sample_field_element; gamma = sample_field_element.
              T_0 = sum_c lambda^c t_c, E_0 = sum_j gamma^j eq(., z_j), claim_0 = sum_j gamma^j sum_c lambda^c v[j][c]; the virtual
              layer F_0 = sum_c lambda^c F_0^c is never committed.  Rounds r = 0 .. R-1 as mlpcs_ref.prove runs them: (r >= 1: commit F_r
              over its two column views, absorb root_r); absorb h_r(0), h_r(1), h_r(2) of sum T_r E_r; draw beta_r; fold T, E and F at
              beta_r.  final and the query indices as in mlpcs_ref
  proof       h_0 | for r = 1..R-1: root_r, h_r | final | per query, per round: round 0 the commitment's row of 2k elements and its path
              of n + b - 1 digests, round r >= 1 two elements and the path.  The values are public, beside the proof
  verify      exact length; canonical elements; the transcript rebuilt; h_r(0) + h_r(1) = claim_r, claim_{r+1} = h_r(beta_r);
              claim_R = sum_j gamma^j (prod_{r<R} eq1(beta_r, z_{j,r})) evaluate_slice(f, final, z_j[R:]); per query the round-0 row
              against the commitment's root, the pair that enters the first fold (sum_c lambda^c row[2c], sum_c lambda^c row[2c+1]),
              from there as mlpcs_ref.verify does
  the device  leaves of a round, per point j, S_X^j = sum_x' T_r[X 2^(n-r-1) + x'] eq(x', z_j[r+1:]), X = 0, 1 (eq_sums_many); the host
              makes h_r = sum_j c_r^j sums_to_round(S_0^j, S_1^j, 1, z_{j,r}) with c_r^j = gamma^j prod_{i<r} eq1(beta_i, z_{j,i})
              (round_from_sums below; tests/test_mlbatch_host.py holds it equal to the direct sums of T E)"""
import random

import cmle_ref
import fri_ref
import merkle_ref
import mlpcs_ref
from oracle import binding as orc

MAX_TABLES, MAX_POINTS = 256, 16
# ---- the kernels' shape (zk_amd/csrc/mlbatch_kernels.cuh; tests/test_mlbatch_host.py asserts these against the header) -----------------
POINTS_PER_PASS = 4                      # kMlPointsPerPass: the Lo tables (2^LO_BITS elements each) of so many points sit in LDS at once
LO_BITS = mlpcs_ref.LO_BITS              # kMlLoBits, shared with the single-point round kernel
# zk_mle_lincomb: a thread takes LINCOMB_ELEMS_PER_THREAD elements per trip of its grid-stride loop (a wave: a run of 64 consecutive
# elements), on at most LINCOMB_MAX_BLOCKS workgroups of mlpcs_ref.THREADS threads; tables below one run go one element per thread
LINCOMB_ELEMS_PER_THREAD, LINCOMB_MAX_BLOCKS = 1, 16384   # kLincombPerThread, kLincombMaxGrid


def lincomb_trips(n):
    """the trips of the grid-stride loop of a lincomb over tables of n variables"""
    blocks = min(-(-(1 << n) // (mlpcs_ref.THREADS * LINCOMB_ELEMS_PER_THREAD)), LINCOMB_MAX_BLOCKS)
    return -(-(1 << n) // (blocks * mlpcs_ref.THREADS * LINCOMB_ELEMS_PER_THREAD))


LINCOMB_SECOND_TRIP_VARS = next(n for n in range(41) if lincomb_trips(n) == 2)   # 23: 2^23 elements on 2^22 threads
LINCOMB_VARS = (0, 1, 5, 6, 7, 13)       # in full against Python integers: below one run, one run, two, many workgroups
LINCOMB_COUNTS = (1, 2, 3, 8)

KM = ((1, 1), (2, 1), (3, 2), (5, POINTS_PER_PASS + 1))


def hash_case(case):
    n, b, f, q, k, m = case
    return mlpcs_ref.hash_case((n, b, f, q)) * 31 + 7 * k + m


def _kept(case):
    """the thinning: one (k, m) in four by the case's hash, so that the host test runs in about the time tests/test_mlpcs_host.py does"""
    n, b, f, q, k, m = case
    return (n + b + f // 2 + (q == 8) + KM.index((k, m))) % 4 == 0


ALL_CASES = tuple((n, b, f, q) + km for n in range(1, 9) for b in (1, 2) for f in (0, 2) if f < n for q in (1, 8) for km in KM)
CASES = tuple(cs for cs in ALL_CASES if _kept(cs))
EQUAL_POINTS_CASE = next(cs for cs in CASES if cs[5] == 2 and cs[0] >= 3)    # its two points are equal
# what the GPU test adds: layer 0 past FRI's power-table split with more points than one pass; a 34-column row
GPU_EXTRA_CASES = ((11, 1, 2, 8, 3, 2), (12, 2, 0, 8, 2, POINTS_PER_PASS + 1), (13, 1, 1, 1, 5, 1), (6, 1, 0, 8, 17, 1))
GPU_CASES = tuple(cs for cs in CASES if cs[3] == 8) + GPU_EXTRA_CASES

be32 = mlpcs_ref.be32


def case_field(case):
    return hash_case(case) % 3


def proof_bytes(n, b, f, q, k, m=1):
    rounds = n - f
    per_query = (2 * k + n + b - 1) + sum(2 + n + b - 1 - r for r in range(1, rounds))
    return 32 * (3 * rounds + rounds - 1 + (1 << f)) + 32 * q * per_query


def lincomb(tables, coeffs, p):
    return [sum(cf * t[i] for cf, t in zip(coeffs, tables)) % p for i in range(len(tables[0]))]


def powers(x, count, p):
    out, cur = [], 1
    for _ in range(count):
        out.append(cur)
        cur = cur * x % p
    return out


def eq_sums_many(t, tails, p):
    """[(S_0^j, S_1^j)] of one table at the tails of m points"""
    return [mlpcs_ref.eq_sums(t, tail, p) for tail in tails]


def round_from_sums(sums, scales, zr, p):
    """h(0), h(1), h(2) from the per-point device sums: sum_j sums_to_round(S_0^j, S_1^j, c^j, z_{j,r})"""
    h = [0, 0, 0]
    for (s0, s1), cj, z in zip(sums, scales, zr):
        h = [(a + x) % p for a, x in zip(h, mlpcs_ref.sums_to_round(s0, s1, cj, z, p))]
    return h


def commit(field, tables, b, shift, layer0s=None):
    """(the k layers F_0^c, the 2k column views, the tree's levels); layer0s: {c: another F_0^c than the table's}, a cheating prover"""
    p, n = fri_ref.modulus(field), len(tables[0]).bit_length() - 1
    assert 1 <= len(tables) <= MAX_TABLES and n >= 1 and all(len(t) == 1 << n for t in tables)
    layers = []
    for c, t in enumerate(tables):
        if layer0s and c in layer0s:
            layers.append(list(layer0s[c]))
        else:
            nv, coeffs = cmle_ref.interpolate_fast(list(t), p)
            layers.append(fri_ref.lde(field, coeffs, n + b, shift))
        assert len(layers[-1]) == 1 << (n + b)
    m0 = 1 << (n + b - 1)
    cols = [half for layer in layers for half in (layer[:m0], layer[m0:])]
    return layers, cols, merkle_ref.commit(cols)


def _start(field, n, b, f, q, k, m, shift, seed, root, points, values):
    assert len(seed) == 32 and len(root) == 32 and len(points) == m and len(values) == m
    tr = orc.Transcript()
    tr.append(seed)
    tr.append(b"".join(int(x).to_bytes(8, "big") for x in (field, n, b, f, q, k, m)))
    tr.append(be32(shift))
    tr.append(root)
    tr.append(b"".join(be32(x) for z in points for x in z))
    tr.append(b"".join(be32(x) for row in values for x in row))
    lam = orc.to_int(field, tr.sample_field_element(field))
    gam = orc.to_int(field, tr.sample_field_element(field))
    return tr, lam, gam


def prove(field, tables, b, f, q, shift, seed, points, sumcheck_tables=None, layer0s=None, values=None, committed=None):
    """(values, proof); values[j][c] = t_c(z_j).  sumcheck_tables: the sumcheck runs on these tables, not on the committed ones;
    layer0s: see commit; values: the matrix that is claimed (and absorbed) whatever the tables give -- three cheating provers.
    committed: what commit() returned, when the caller has it"""
    p, n, k, m = fri_ref.modulus(field), len(tables[0]).bit_length() - 1, len(tables), len(points)
    assert 1 <= b <= mlpcs_ref.MAX_BLOWUP_LOG and 0 <= f < n and 1 <= q <= mlpcs_ref.MAX_QUERIES and shift % p and 1 <= m <= MAX_POINTS
    layers0, cols0, levels0 = committed or commit(field, tables, b, shift, layer0s)
    ts = [[x % p for x in t] for t in (sumcheck_tables if sumcheck_tables is not None else tables)]
    points = [[x % p for x in z] for z in points]
    assert all(len(z) == n for z in points)
    if values is None:
        values = [[mlpcs_ref.evaluate(t, z, p) for t in ts] for z in points]
    tr, lam, gam = _start(field, n, b, f, q, k, m, shift, seed, merkle_ref.root(levels0), points, values)
    lp, gp = powers(lam, k, p), powers(gam, m, p)
    t = lincomb(ts, lp, p)
    e = lincomb([mlpcs_ref.eq_table(z, p) for z in points], gp, p)
    layer = lincomb(layers0, lp, p)          # virtual: never committed
    s, rounds = shift, n - f
    layers, trees, out = [cols0], [levels0], b""
    for r in range(rounds):
        if r >= 1:
            half = len(layer) // 2
            cols = [layer[:half], layer[half:]]
            levels = merkle_ref.commit(cols)
            layers.append(cols)
            trees.append(levels)
            tr.append(merkle_ref.root(levels))
            out += merkle_ref.root(levels)
        h = b"".join(be32(x) for x in mlpcs_ref.round_sums(t, e, p))
        tr.append(h)
        out += h
        beta = orc.to_int(field, tr.sample_field_element(field))
        t, e = mlpcs_ref.partial_evaluate0(t, beta, p), mlpcs_ref.partial_evaluate0(e, beta, p)
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
        idx = mlpcs_ref._query_index(tr, m0)
        for r in range(rounds):
            row, path = merkle_ref.open(trees[r], layers[r], idx % (m0 >> r))
            out += b"".join(be32(x) for x in row) + b"".join(path)
    assert len(out) == proof_bytes(n, b, f, q, k, m)
    return values, out


def verify(field, n, b, f, q, k, shift, seed, root, points, values, proof):
    p, m = fri_ref.modulus(field), len(points)
    if not (1 <= k <= MAX_TABLES and 1 <= m <= MAX_POINTS) or len(proof) != proof_bytes(n, b, f, q, k, m) or len(values) != m:
        return False
    if any(len(z) != n or any(not 0 <= x < p for x in z) for z in points) or any(len(row) != k or any(not 0 <= x < p for x in row) for row in values):
        return False
    rounds = n - f
    tr, lam, gam = _start(field, n, b, f, q, k, m, shift, seed, root, points, values)
    lp, gp = powers(lam, k, p), powers(gam, m, p)
    claim = sum(gp[j] * sum(lp[c] * values[j][c] for c in range(k)) for j in range(m)) % p
    roots, betas, at = [root], [], 0

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
        claim = mlpcs_ref.quadratic_at(h, betas[-1], p)
    final_at = at
    final = elems(1 << f)
    if any(x >= p for x in final):
        return False
    tr.append(proof[final_at:at])
    want = 0
    for j, z in enumerate(points):
        scale = gp[j]
        for r in range(rounds):
            scale = scale * mlpcs_ref.eq1(betas[r], z[r], p) % p
        want = (want + scale * cmle_ref.evaluate_slice(f, final, z[rounds:], p)) % p
    if claim != want:
        return False
    m0 = 1 << (n + b - 1)
    for _ in range(q):
        idx = mlpcs_ref._query_index(tr, m0)
        y, s = None, shift
        for r in range(rounds):
            mr = m0 >> r
            rho = idx % mr
            width = 2 * k if r == 0 else 2
            row = elems(width)
            log_m = mr.bit_length() - 1
            path = [proof[at + 32 * j:at + 32 * j + 32] for j in range(log_m)]
            at += 32 * log_m
            if any(x >= p for x in row) or not merkle_ref.verify(roots[r], log_m, width, rho, row, path):
                return False
            if r == 0:   # the pair of the virtual layer 0
                row = [sum(lp[c] * row[2 * c + x] for c in range(k)) % p for x in range(2)]
            elif row[idx // mr] != y:
                return False
            x = s * pow(fri_ref.root(field, 2 * mr), rho, p) % p
            y = fri_ref.fold(field, row, x, betas[r], 1)[0]
            idx, s = rho, s * s % p
        x = s * pow(fri_ref.root(field, m0 >> (rounds - 1)), idx, p) % p
        g = 0
        for cj in reversed(final):
            g = (g * x + cj) % p
        if g != y:
            return False
    return True


def section_offsets(n, b, f, q, k, m=1):
    """byte offsets of one element of each section of a proof: an h, a root (None when R = 1), a final coefficient, a round-0 row element
    in an even and in an odd column, a later row element (None when R = 1), a path digest"""
    rounds = n - f
    head = 32 * (3 * rounds + rounds - 1)
    q0 = head + (32 << f)
    later = q0 + 32 * (2 * k + n + b - 1)
    return {"h": 32, "root": 96 if rounds > 1 else None, "final": head, "row_even": q0 + 64 * (k - 1), "row_odd": q0 + 64 * (k - 1) + 32,
            "row_later": later + 32 if rounds > 1 else None, "path": q0 + 64 * k}


def case_tables(p, field_index, n, k, worst_case_values):
    """k different tables of 2^n canonical ints: consecutive slices of fri_ref.fold_input's worst-case mix"""
    big = fri_ref.fold_input(p, field_index, n + max(k - 1, 0).bit_length(), worst_case_values)
    return [big[c << n:(c + 1) << n] for c in range(k)]


def case_inputs(field_index, case, worst_case_values):
    """(tables, shift, seed, points) of a shared case: the shift in {1, 5, p - 1, random}, the entries of the points in {0, 1, p - 1,
    random} by their place; EQUAL_POINTS_CASE has two equal points"""
    n, b, f, q, k, m = case
    p = fri_ref.modulus(field_index)
    rng = random.Random(0xBA7C + 1000 * field_index + hash_case(case))
    tables = case_tables(p, field_index, n, k, worst_case_values)
    shift = (1, 5, p - 1, rng.randrange(1, p))[hash_case(case) % 4]
    seed = bytes(rng.randrange(256) for _ in range(32))
    points = [[mlpcs_ref.point_entries(p, rng)[(hash_case(case) // 4 + 3 * i + j) % 4] for i in range(n)] for j in range(m)]
    if case == EQUAL_POINTS_CASE:
        points[1] = list(points[0])
    return tables, shift, seed, points


def eq_sums_many_case(field_index, n, n_points, worst_case_values):
    """(table, tails) of one device zk_mle_eq_sums_many case: point 0's tail is mlpcs_ref.eq_sums_case's (0, 1 and p - 1 from n = 8 on)"""
    p = fri_ref.modulus(field_index)
    table, tail = mlpcs_ref.eq_sums_case(field_index, n, worst_case_values)
    rng = random.Random(0xE96 + 1000 * field_index + 64 * n + n_points)
    tails = [tail] + [[mlpcs_ref.point_entries(p, rng)[(i + j) % 4] if i % 2 else rng.randrange(p) for i in range(n - 1)] for j in range(1, n_points)]
    return table, tails


def lincomb_case(field_index, n, k, worst_case_values):
    """(tables, coeffs): coefficients in {0, 1, p - 1, random} by their place"""
    p = fri_ref.modulus(field_index)
    rng = random.Random(0x11C0 + 1000 * field_index + 64 * n + k)
    big = fri_ref.fold_input(p, field_index, n + max(k - 1, 0).bit_length(), worst_case_values)
    tables = [big[c << n:(c + 1) << n] for c in range(k)]
    coeffs = [(0, 1, p - 1, rng.randrange(p))[(c + n + k) % 4] for c in range(k)]
    return tables, coeffs
