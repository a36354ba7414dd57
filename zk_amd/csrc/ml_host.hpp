// ml_host.hpp -- the small host helpers that the two multilinear commitments share (mlpcs.hip: one table, one point; mlbatch.hip: k tables,
// m points): the shapes and limits of an opening, the proof's per-query length, and the sumcheck's host arithmetic on the two sums that the
// round kernels leave (tests/mlpcs_ref.py eq1, sums_to_round, quadratic_at).  Host only; on top of host_core.hpp.
#pragma once
#include "host_core.hpp"

constexpr uint32_t kMlMaxBlowupLog = 8, kMlMaxQueries = 1024;   // FRI's limits (fri.hip)

inline size_t ml_scratch_bytes(size_t bytes) {
    size_t b = 32;
    while (b < bytes) b <<= 1;
    return b;
}
inline bool ml_open_shape(uint32_t n, uint32_t b, uint32_t f, uint32_t q) {
    return n >= 1 && n <= kMaxVars && b >= 1 && b <= kMlMaxBlowupLog && f < n && q >= 1 && q <= kMlMaxQueries;
}
// elements and digests of one query: round 0's row of `row0` elements (2 for one table, 2k for k), later rows of 2, every round's path
inline uint64_t ml_per_query(uint32_t n, uint32_t b, uint32_t f, uint32_t row0) {
    const uint32_t R = n - f;
    uint64_t per_query = row0 - 2;
    for (uint32_t r = 0; r < R; ++r) per_query += 2 + n + b - 1 - r;
    return per_query;
}
inline uint64_t ml_proof_bytes(uint32_t n, uint32_t b, uint32_t f, uint32_t q, uint32_t row0 = 2) {
    const uint32_t R = n - f;
    return 32 * (3ull * R + R - 1 + (1ull << f)) + 32ull * q * ml_per_query(n, b, f, row0);
}
// eq1(b, z) = (1 - b)(1 - z) + b z
inline Fe ml_eq1(const Fe &b, const Fe &z, const FieldParams &P) {
    const Fe one = fe_one(P), bz = fe_mul(b, z, P);
    return fe_add(fe_sub(fe_sub(one, b, P), z, P), fe_add(bz, bz, P), P);
}
// h(0), h(1), h(2) = c (1 - z) S_0, c z S_1, c (3 z - 1)(2 S_1 - S_0)
inline void ml_round_poly(const Fe &s0, const Fe &s1, const Fe &c, const Fe &z, const FieldParams &P, Fe h[3]) {
    const Fe one = fe_one(P), z2 = fe_add(z, z, P);
    h[0] = fe_mul(fe_mul(c, fe_sub(one, z, P), P), s0, P);
    h[1] = fe_mul(fe_mul(c, z, P), s1, P);
    h[2] = fe_mul(fe_mul(c, fe_sub(fe_add(z2, z, P), one, P), P), fe_sub(fe_add(s1, s1, P), s0, P), P);
}
// the quadratic through (0, h0), (1, h1), (2, h2) at x: h0 (x-1)(x-2)/2 - h1 x (x-2) + h2 x (x-1)/2
inline Fe ml_quadratic_at(const Fe h[3], const Fe &x, const Fe &half, const FieldParams &P) {
    const Fe one = fe_one(P), x1 = fe_sub(x, one, P), x2 = fe_sub(x1, one, P);
    const Fe a = fe_mul(fe_mul(h[0], fe_mul(x1, x2, P), P), half, P), b = fe_mul(h[1], fe_mul(x, x2, P), P);
    return fe_add(fe_sub(a, b, P), fe_mul(fe_mul(h[2], fe_mul(x, x1, P), P), half, P), P);
}
