"""Big-int definition of zk_upoly_divrem and zk_upoly_inverse_series (the reference has no division, so this file is what parity
means), and the restatement of what the device runs: the Newton inversion, the reversed quotient with the truncated remainder
product, and the linear divisor's affine scan in chunks.  Conventions of univariate_poly.rs: degree() = len - 1 (:88-94), nothing is
ever trimmed, the empty list is the zero polynomial.  All values are canonical ints mod p."""


class ZeroLead(Exception):
    """the coefficient that has to be inverted is zero (the library: ZK_ERR_PANIC_INVERSE)"""


def _inv(v, p):
    if v % p == 0:
        raise ZeroLead()
    return pow(v, p - 2, p)


def mul(a, b, p):   # Mul for &UnivariatePolynomial (:186-209): an empty operand gives the empty product
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % p
    return out


def divrem(a, b, p):
    """schoolbook long division by lengths: (q, r) with a = q b + r, len(q) = la - lb + 1 and len(r) = lb - 1; la < lb: ([], a).
    b empty: ValueError (ZK_ERR_BAD_ARG); b[-1] = 0: ZeroLead"""
    la, lb = len(a), len(b)
    if lb == 0:
        raise ValueError("empty divisor")
    if la < lb:
        return [], list(a)
    inv = _inv(b[-1], p)
    rem = [v % p for v in a]
    k = la - lb + 1
    q = [0] * k
    for j in range(k - 1, -1, -1):
        q[j] = rem[j + lb - 1] * inv % p
        for i in range(lb):
            rem[j + i] = (rem[j + i] - q[j] * b[i]) % p
    return q, rem[:lb - 1]


def inverse_series(f, k, p):
    """1 / f mod z^k by the recurrence g_n = -(sum_{i=1..n} f_i g_{n-i}) / f_0; coefficients of f beyond len(f) are zero"""
    if k == 0:
        return []
    if not f:
        raise ZeroLead()
    inv = _inv(f[0], p)
    g = [inv]
    for n in range(1, k):
        s = sum(f[i] * g[n - i] for i in range(1, min(n, len(f) - 1) + 1)) % p
        g.append((-s * inv) % p)
    return g


def inverse_series_newton(f, k, p):
    """the device's steps: alpha <- alpha (2 - f alpha) mod z^min(2t, k), each product over the coefficients that exist"""
    if k == 0:
        return []
    if not f:
        raise ZeroLead()
    alpha, t = [_inv(f[0], p)], 1
    while t < k:
        n2 = min(2 * t, k)
        fl = min(len(f), n2)
        e = mul(f[:fl], alpha, p)
        g = [((2 if i == 0 else 0) - (e[i] if i < len(e) else 0)) % p for i in range(n2)]
        alpha = mul(alpha, g, p)[:n2]
        t *= 2
    return alpha


def divrem_newton(a, b, p):
    """q = rev_k((rev(a) mod z^k)(1 / rev(b) mod z^k) mod z^k); r[i] = a[i] - (q[0..min(m, k)) b[0..m))[i], i < m = lb - 1"""
    la, lb = len(a), len(b)
    if lb == 0:
        raise ValueError("empty divisor")
    if la < lb:
        return [], list(a)
    k, m = la - lb + 1, lb - 1
    ra = [a[la - 1 - i] for i in range(k)]
    lbk = min(lb, k)
    rb = [b[lb - 1 - i] for i in range(lbk)]
    alpha = inverse_series_newton(rb, k, p)
    prod = mul(ra, alpha, p)
    q = [prod[k - 1 - j] for j in range(k)]
    if not m:
        return q, []
    qb = mul(q[:min(m, k)], b[:m], p)
    return q, [(a[i] - qb[i]) % p for i in range(m)]


def divrem_linear_scan(a, b, p, chunk=8, run=2, lanes=None):
    """lb = 2 by the backward affine scan in chunks: inv = 1/b1, z = -b0 inv, S[i] = a[i] + z S[i+1]; q[j] = inv S[j+1], r[0] = S[0].
    Per chunk the Horner total H_c over lane runs of `run` coefficients (missing ones count as 0), then the carries
    carry_c = carry_(c+1) z^chunk + H_(c+1) (0 for the top chunk) and the chunks again, the carry entering the last lane's run"""
    assert len(b) == 2 and len(a) >= 2 and chunk % run == 0
    la = len(a)
    lanes = chunk // run
    inv = _inv(b[1], p)
    z = (-b[0] * inv) % p
    nc = (la + chunk - 1) // chunk
    at = lambda i: a[i] if i < la else 0   # noqa: E731

    def lane_values(c):
        return [sum(at(c * chunk + l * run + u) * pow(z, u, p) for u in range(run)) % p for l in range(lanes)]

    def suffix(h):   # V[t] = sum_{l >= t} h_l z^(run (l - t)), Hillis-Steele from the top with the step squared a level
        v, w, d = list(h), pow(z, run, p), 1
        while d < lanes:
            v = [(v[t] + v[t + d] * w) % p if t + d < lanes else v[t] for t in range(lanes)]
            w, d = w * w % p, 2 * d
        return v

    H = [suffix(lane_values(c))[0] for c in range(nc)]
    carry, Z = [0] * nc, pow(z, chunk, p)
    for c in range(nc - 2, -1, -1):
        carry[c] = (carry[c + 1] * Z + H[c + 1]) % p
    q = [0] * (la - 1)
    for c in range(nc):
        h = lane_values(c)
        h[lanes - 1] = (h[lanes - 1] + carry[c] * pow(z, run, p)) % p
        v = suffix(h)
        for l in range(lanes):
            cur = v[l + 1] if l + 1 < lanes else carry[c]
            for u in range(run - 1, -1, -1):
                i = c * chunk + l * run + u
                if i >= la:
                    continue
                cur = (cur * z + a[i]) % p
                if i:
                    q[i - 1] = cur * inv % p
    r0 = (H[0] + carry[0] * Z) % p if nc else 0
    return q, [r0]
