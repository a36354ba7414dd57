"""What tests/test_gpu_upoly.py and tests/upoly_structured_check.py check univariate products with: the schoolbook product on
Python integers and the shipped cost model's crossover."""
from oracle import binding as orc


def direct_up_to(total):
    """largest min(la, lb) the shipped cost model (ntt.hip upoly_direct) sends to the direct kernel at la + lb = total"""
    return max(m for m in range(1, total) if max(0.7 * m, 9e-6 * m * total) <= 95.0 + 3.5e-4 * total)


def schoolbook(field, a, b):
    """Mul for &UnivariatePolynomial (univariate_poly.rs:186-209) on canonical Python ints"""
    p = orc.modulus(field)
    if not a or not b:
        return []
    if len(a) > len(b):
        a, b = b, a
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return [v % p for v in out]
