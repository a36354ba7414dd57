"""Python restatements (canonical big ints) of UnivariatePolynomial::interpolate_xy and Add (polynomial/src/univariate_poly.rs)
for the interpolation tests: `lagrange_literal` follows the reference's loops, `lagrange` is the same sum in O(n^2)."""


class RefPanic(Exception):
    """where the reference panics: (x_i - x_j).inverse().unwrap() on a zero difference (univariate_poly.rs:68)"""


def add(a, b, p):   # Add for &UnivariatePolynomial (:157-184): empty -> the other; else max length, nothing trimmed
    if not a:
        return list(b)
    if not b:
        return list(a)
    out = list(a) if len(a) >= len(b) else list(b)
    short = b if len(a) >= len(b) else a
    for i, v in enumerate(short):
        out[i] = (out[i] + v) % p
    return out


def mul(a, b, p):   # Mul (:186-209)
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % p
    return out


def lagrange_literal(xs, ys, p):   # interpolate_xy (:54-80), loop for loop
    result = []
    for i, (x, y) in enumerate(zip(xs, ys)):
        basis = [1]
        for j, xj in enumerate(xs):
            if j == i:
                continue
            d = (x - xj) % p
            if d == 0:
                raise RefPanic(i, j)
            basis = mul(basis, mul([(-xj) % p, 1], [pow(d, p - 2, p)], p), p)
        result = add(result, mul(basis, [y % p], p), p)
    return result


def lagrange(xs, ys, p):
    """the same sum as sum_i w_i M(x) / (x - x_i), M = prod_j (x - x_j) over all nx points, w_i = y_i / prod_{j != i}(x_i - x_j)"""
    nx, m = len(xs), min(len(xs), len(ys))
    if m == 0:
        return []
    M = [1]
    for xj in xs:   # M *= (x - xj), coefficients lowest first
        M = [((M[k - 1] if k else 0) - xj * (M[k] if k < len(M) else 0)) % p for k in range(len(M) + 1)]
    out = [0] * nx
    for i in range(m):
        d = 1
        for j in range(nx):
            if j != i:
                d = d * (xs[i] - xs[j]) % p
        if d == 0:
            raise RefPanic(i)
        w = ys[i] * pow(d, p - 2, p) % p
        q, carry = [0] * nx, 0   # M / (x - x_i) by synthetic division, highest first
        for k in range(nx, 0, -1):
            carry = (M[k] + carry * xs[i]) % p if k < nx else M[k]
            q[k - 1] = carry
        for k in range(nx):
            out[k] = (out[k] + w * q[k]) % p
    return out
