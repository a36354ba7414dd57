// inv_field.cuh -- one field inversion by the binary extended Euclidean algorithm, for the batch inversion's single inverse per call
// (inv_kernels.cuh).  fe_inverse_dev (upoly_kernels.cuh) is Fermat: ~380 DEPENDENT Montgomery multiplications on one lane, 0.56 ms on the
// MI355X whatever the table's size (profiles/batch_inverse.log); this takes at most 2 * 256 rounds of 8-limb shifts, additions and
// subtractions and two multiplications.  Host and device: tests/cpp/test_inverse_host.cpp compares it with the host's Fermat inverse.
// The inverse is unique, so both give the same bits.
#pragma once
#include "field.cuh"

namespace zk {

// x / 2 mod p for x < p (p odd, p < 2^255: x + p does not leave eight limbs)
ZK_HD void inv_half_mod(uint32_t x[8], const uint32_t p[8]) {
    if (x[0] & 1u) add8(x, x, p);
#pragma unroll
    for (int i = 0; i < 7; ++i) x[i] = (x[i] >> 1) | (x[i + 1] << 31);
    x[7] >>= 1;
}
ZK_HD void inv_shr1(uint32_t x[8]) {
#pragma unroll
    for (int i = 0; i < 7; ++i) x[i] = (x[i] >> 1) | (x[i + 1] << 31);
    x[7] >>= 1;
}
ZK_HD bool inv_is_one(const uint32_t x[8]) {
    uint32_t rest = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i) rest |= x[i];
    return x[0] == 1u && rest == 0;
}
// a^-1 in Montgomery form for a in Montgomery form (0 -> 0).  The loop works on the stored integer A = a R mod p and ends with
// A^-1 mod p = a^-1 R^-1; two multiplications by R^2 bring it to a^-1 R.  Invariants: x1 A = u and x2 A = v (mod p), gcd(u, v) = 1.
ZK_HD Fe fe_inverse_binary(const Fe &a, const FieldParams &P) {
    if (fe_is_zero(a)) return a;
    Fe u = a, v, x1, x2 = fe_zero();
#pragma unroll
    for (int i = 0; i < 8; ++i) v.v[i] = P.p[i], x1.v[i] = i == 0 ? 1u : 0u;
    while (!inv_is_one(u.v) && !inv_is_one(v.v)) {
        while (!(u.v[0] & 1u)) {
            inv_shr1(u.v);
            inv_half_mod(x1.v, P.p);
        }
        while (!(v.v[0] & 1u)) {
            inv_shr1(v.v);
            inv_half_mod(x2.v, P.p);
        }
        uint32_t d[8];
        if (sub8(d, u.v, v.v) == 0) {   // u >= v
#pragma unroll
            for (int i = 0; i < 8; ++i) u.v[i] = d[i];
            x1 = fe_sub(x1, x2, P);
        } else {
            (void)sub8(v.v, v.v, u.v);
            x2 = fe_sub(x2, x1, P);
        }
    }
    const Fe x = inv_is_one(u.v) ? x1 : x2;
    Fe r2;
#pragma unroll
    for (int i = 0; i < 8; ++i) r2.v[i] = P.r2[i];
    return fe_mul(fe_mul(x, r2, P), r2, P);
}

}  // namespace zk
