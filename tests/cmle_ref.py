"""Python restatements (canonical big ints, dicts for the reference's BTreeMap) of CoeffMultilinearPolynomial::interpolate,
evaluate_slice and to_bytes (polynomial/src/multilinear/coefficient_form.rs) for the coefficient-form tests.

`interpolate_literal` follows the reference loop for loop: one lagrange_basis_poly per value built by map products (Mul :375-412,
zero coefficients skipped), scalar_multiply (:272-281, nothing dropped) and the map Add (:350-373: the longer map cloned, the shorter
summed in).  `interpolate_fast` is the same result as an O(n 2^n) Moebius transform of the zero-padded table plus a bit reversal."""


def bit_count_for_n_elem(size):   # :517-523: len(format!("{:b}", size - 1))
    return len(format(size - 1, "b"))


def binary_string(index, bit_count):   # :461-464
    b = format(index, "b")
    return "0" * max(bit_count - len(b), 0) + b


def selector_from_usize(value, exact_size):   # :432-446
    bits = [ch == "1" for ch in format(value, "b")]
    bits.reverse()
    return (bits + [False] * exact_size)[:exact_size] if len(bits) < exact_size else bits[:exact_size]


def selector_to_index(selector):   # :418-430
    return sum(1 << i for i, b in enumerate(selector) if b)


# a polynomial is (n_vars, {key: coefficient})
def _mul(a, b, p):   # Mul for &CoeffMultilinearPolynomial (:375-412)
    (na, ca), (nb, cb) = a, b
    if na == 0:
        return scalar_multiply(b, ca.get(0, 0), p)
    if nb == 0:
        return scalar_multiply(a, cb.get(0, 0), p)
    out = {}
    for i, x in sorted(ca.items()):
        for j, y in sorted(cb.items()):
            if x == 0 or y == 0:
                continue
            key = selector_to_index(selector_from_usize(i, na) + selector_from_usize(j, nb))
            out[key] = (out.get(key, 0) + x * y) % p
    return (na + nb, out)


def scalar_multiply(a, s, p):   # :272-281
    return (a[0], {k: v * s % p for k, v in a[1].items()})


def _add(a, b, p):   # Add (:350-373)
    (na, ca), (nb, cb) = a, b
    n, longer, shorter = (na, dict(ca), cb) if len(ca) > len(cb) else (nb, dict(cb), ca)
    for k, v in shorter.items():
        longer[k] = (longer.get(k, 0) + v) % p
    return (n, longer)


def _check_zero(p):   # 1 - a (:256-263)
    return (1, {0: 1, 1: p - 1})


def _check_one():   # a (:266-269)
    return (1, {1: 1})


def lagrange_basis_poly(index, n_vars, p):   # :218-237
    acc = (0, {0: 1})   # multiplicative_identity (:335-337)
    for ch in binary_string(index, n_vars):
        acc = _mul(acc, _check_one() if ch == "1" else _check_zero(p), p)
    return acc


def interpolate_literal(values, p):   # :200-216 -> (n_vars, {key: coefficient})
    if not values:
        return (0, {})
    n = bit_count_for_n_elem(len(values))
    result = (0, {})   # additive_identity
    for i, v in enumerate(values):
        result = _add(result, scalar_multiply(lagrange_basis_poly(i, n, p), v, p), p)
    return result


def interpolate_fast(values, p):   # the same as a dense vector in key order: (n_vars, [2^n_vars coefficients])
    if not values:
        return (0, [])
    n = bit_count_for_n_elem(len(values))
    t = [v % p for v in values] + [0] * ((1 << n) - len(values))
    for b in range(n):   # Moebius: T[x | 2^b] -= T[x]
        for x in range(1 << n):
            if x >> b & 1:
                t[x] = (t[x] - t[x ^ (1 << b)]) % p
    rev = lambda k: int(format(k, f"0{n}b")[::-1], 2)  # noqa: E731  table index bit n-1-v <-> key bit v
    return (n, [t[rev(k)] for k in range(1 << n)])


def evaluate_slice(n_vars, dense, point, p):   # :39-69 over a dense vector; point: canonical ints
    if n_vars == 0:
        return dense[0] if dense else 0
    if len(point) < n_vars:
        raise ValueError("evaluate requires an assignment for every variable")
    acc = 0
    for k, ck in enumerate(dense):
        term = ck
        for v in range(n_vars):
            if k >> v & 1:
                term = term * point[v] % p
        acc = (acc + term) % p
    return acc


def to_bytes(n_vars, dense):   # :131-139
    out = bytearray(n_vars.to_bytes(4, "big"))
    for k, ck in enumerate(dense):
        out += k.to_bytes(8, "big") + ck.to_bytes(32, "big")
    return bytes(out)
