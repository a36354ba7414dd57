"""Python restatement (canonical big ints, dicts for the reference's BTreeMap) of the algebra of CoeffMultilinearPolynomial
(polynomial/src/multilinear/coefficient_form.rs): partial_evaluate with get_variable_indexes, relabel with its presence vector and
key remapping, Add and scalar_multiply, loop for loop.  A polynomial is (n_vars, {key: coefficient}) as in tests/cmle_ref.py, whose
_mul is the Mul of this model.  Errors are ValueError with the reference's text."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cmle_ref import _mul, selector_from_usize, selector_to_index  # noqa: E402,F401

SELECTOR_LEN_TEXT = "the selector array len should be the same as the number of variables"
SELECTOR_SINGLE_TEXT = "only select single variable, cannot get indexes for constant or multiple variables"


def new(n_vars, terms, p):   # ::new :158-176: [(coefficient, selector)], duplicate selectors summed
    co = {}
    for coeff, selector in terms:
        if len(selector) != n_vars:
            raise ValueError(SELECTOR_LEN_TEXT)
        k = selector_to_index(selector)
        co[k] = (co.get(k, 0) + coeff) % p
    return (n_vars, co)


def get_variable_indexes(n_vars, selector):   # :285-327
    if len(selector) != n_vars:
        raise ValueError(SELECTOR_LEN_TEXT)
    if sum(1 for s in selector if s) != 1:
        raise ValueError(SELECTOR_SINGLE_TEXT)
    variable_id = selector_to_index(selector)
    indexes, count, skip = [], 0, False
    for i in range(variable_id, 1 << n_vars):
        if count == variable_id:
            skip = not skip
            count = 0
        if not skip:
            indexes.append(i)
        count += 1
    return indexes


def partial_evaluate(poly, assignments, p):   # :72-104; assignments: [(selector, value)]
    n_vars, co = poly[0], dict(poly[1])
    for selector, value in assignments:
        if len(selector) > n_vars:
            continue
        for i in get_variable_indexes(n_vars, selector):
            if i in co:
                old = co.pop(i)
                j = i - selector_to_index(selector)
                co[j] = (co.get(j, 0) + old * value) % p
    return (n_vars, co)


def variable_presence_vector(poly):   # :243-253
    acc = [False] * poly[0]
    for key in poly[1]:
        acc = [a | b for a, b in zip(acc, selector_from_usize(key, poly[0]))]
    return acc


def mapping_instruction_from_variable_presence(presence):   # :469-483
    next_var, mapping = 0, []
    for index, is_present in enumerate(presence):
        if is_present:
            if next_var != index:
                mapping.append((index, next_var))
            next_var += 1
    return mapping


def relabel(poly, p):   # :109-123 with remap_coefficient_keys :494-514
    n_vars, co = poly[0], dict(poly[1])
    if n_vars == 0:
        return (n_vars, co)
    presence = variable_presence_vector(poly)
    for a, b in mapping_instruction_from_variable_presence(presence):
        old_var, new_var = 1 << a, 1 << b   # to_power_of_two :486-491
        for index in get_variable_indexes(n_vars, selector_from_usize(old_var, n_vars)):
            if index in co:
                coeff = co.pop(index)
                j = index - old_var + new_var
                co[j] = (co.get(j, 0) + coeff) % p
    return (sum(1 for x in presence if x), co)


def add(a, b, p):   # Add :350-373
    (na, ca), (nb, cb) = a, b
    n, longer, shorter = (na, dict(ca), cb) if len(ca) > len(cb) else (nb, dict(cb), ca)
    for k, v in shorter.items():
        longer[k] = (longer.get(k, 0) + v) % p
    return (n, longer)


def scalar_multiply(a, s, p):   # :272-282
    return (a[0], {k: v * s % p for k, v in a[1].items()})


def mul(a, b, p):   # Mul :375-415
    return _mul(a, b, p)


def to_bytes(poly):   # :131-139 of a map
    out = bytearray(poly[0].to_bytes(4, "big"))
    for k in sorted(poly[1]):
        out += k.to_bytes(8, "big") + poly[1][k].to_bytes(32, "big")
    return bytes(out)


def evaluate_slice(poly, point, p):   # :39-69: every variable assigned in order, then the coefficient of key 0
    n_vars = poly[0]
    if n_vars == 0:
        return poly[1].get(0, 0)
    if len(point) < n_vars:
        raise ValueError("evaluate requires an assignment for every variable")
    sel = lambda v: [i == v for i in range(n_vars)]  # noqa: E731  selector_from_position :450-458
    return partial_evaluate(poly, [(sel(v), point[v]) for v in range(n_vars)], p)[1][0]


def selector(n_vars, v):
    return [i == v for i in range(n_vars)]
