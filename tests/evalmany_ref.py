"""Python restatement (canonical big ints) of the transposed subproduct tree behind zk_upoly_evaluate_many's tree path (DESIGN.md
section 11; Bostan, Lecerf, Schost, ISSAC 2003), step for step as the device runs it, and Horner (univariate_poly.rs:29-40) to hold
it against.  `stop` is the node size at which the recursion hands over to the bottom formula (the device: 2^7)."""


def horner(coeffs, x, p):   # UnivariatePolynomial::evaluate (:29-40)
    acc = 0
    for co in reversed(coeffs):
        acc = (acc * x + co) % p
    return acc


def horner_many(coeffs, xs, p):
    return [horner(coeffs, x, p) for x in xs]


def _mul(a, b, p):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % p
    return out


def _cyclic(a, b, size, p):   # cyclic convolution of `size` points (b shorter: padded with zeros)
    out = [0] * size
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[(i + j) % size] = (out[(i + j) % size] + x * y) % p
    return out


def up_sweep(xs, p, stop=1):
    """levels[l] = the m-arrays of the nodes of 2^l points (monic node polynomials without the leading 1), concatenated, for
    2^l = stop .. N; a node combines as m = x^s (m_L + m_R) + m_L m_R"""
    N = len(xs)
    cur, s = [(-x) % p for x in xs], 1
    levels = {0: cur}
    while s < N:
        nxt = []
        for b in range(0, N, 2 * s):
            ml, mr = cur[b:b + s], cur[b + s:b + 2 * s]
            prod = _mul(ml, mr, p) + [0]
            node = [(prod[k] + (ml[k - s] + mr[k - s] if k >= s else 0)) % p for k in range(2 * s)]
            nxt += node
        cur, s = nxt, 2 * s
        levels[s.bit_length() - 1] = cur
    return levels


def invert_series(R, N, p):
    """alpha = 1/R mod z^N, R_0 = 1, by Newton steps alpha <- alpha (2 - R alpha) mod z^(2t)"""
    alpha, t = [1], 1
    while t < N:
        e = _mul(R[:2 * t], alpha, p)[:2 * t]
        g = [(2 - e[0]) % p] + [(-v) % p for v in e[1:]]
        alpha = _mul(alpha, g, p)[:2 * t]
        t *= 2
    return alpha[:N]


def evaluate_many_tree(coeffs, xs, p, stop=1):
    n, L = len(xs), len(coeffs)
    if n == 0:
        return []
    N = 1
    while N < max(n, L, 1):
        N *= 2
    stop = min(stop, N)
    xp = [x % p for x in xs] + [0] * (N - n)                       # 1. pad: the padded points are zeros, their outputs dropped
    c = [v % p for v in coeffs] + [0] * (N - L)
    levels = up_sweep(xp, p)                                       # 2. every level kept
    log_N = N.bit_length() - 1
    m_root = levels[log_N]
    R = [1] + [m_root[N - k] for k in range(1, N)]                 # 3. R = rev(M) mod z^N
    alpha = invert_series(R, N, p)
    prod = _mul(c[::-1], alpha, p)[:N]                             # 4. b = reversal of the first N coefficients of rev(c) alpha
    b = prod[::-1]
    s = N // 2                                                     # 5. down-sweep
    while 2 * s > stop:
        m = levels[s.bit_length() - 1]
        nxt = [0] * N
        for base in range(0, N, 2 * s):
            node = b[base:base + 2 * s]
            ml, mr = m[base:base + s], m[base + s:base + 2 * s]
            cl, cr = _cyclic(node, mr, 2 * s, p), _cyclic(node, ml, 2 * s, p)
            for j in range(s):
                nxt[base + j] = (node[j] + cl[s + j]) % p
                nxt[base + s + j] = (node[j] + cr[s + j]) % p
        b, s = nxt, s // 2
    s = stop                                                       # 6. bottom: out_i = sum_k b_k q_k, q_0 = 1, q_k = R_k + x_i q_(k-1)
    m = levels[s.bit_length() - 1]
    out = []
    for i in range(n):
        base = i - i % s
        q, acc = 1, b[base]
        for k in range(1, s):
            q = (m[base + s - k] + xp[i] * q) % p
            acc = (acc + b[base + k] * q) % p
        out.append(acc)
    return out
