// fri_kernels.cuh -- gfx950 kernels of the FRI low-degree proofs (no reference item; definition: tests/fri_ref.py; host side: fri.hip;
// DESIGN.md section 14).
//
// A layer is 2^n evaluations over the coset s * <w_N> in NATURAL order, so a fold by 2^A reads, for output i < M = N / 2^A, the 2^A
// inputs v[i + j M]: 2^A coalesced streams of 32-byte elements, the MSB fold's access pattern (kernels.cuh k_fold_msb) with a per-element
// multiplier.  The A butterfly levels run in registers:
//   level l, butterfly j < 2^(A-1-l):   x[j] <- (x[j] + x[j + h]) + (x[j] - x[j + h]) * w_{2^A}^(-2^l j) * U_l,     h = 2^(A-1-l)
//   U_0 = (beta / s) * w_N^-i            per lane: w_N^-i from a two-level power table, beta / s prepared on the host (Mul29, SGPRs)
//   U_l = U_{l-1}^2                      = (beta / s)^(2^l) * w_N^(-2^l i): the squaring carries the level's challenge and shift along
//   w_{2^A}^-1, ^-2, ^-3                 wave-uniform, prepared on the host; butterfly 0 of every level needs none
// and the halves of all levels are taken at the end as A halvings of the one output (fe_half: a conditional add of p and a shift; exact
// arithmetic, so the same canonical element as fri_ref.fold's level-by-level halves).  Multiplications per output: 1 (table compose; none
// up to 2^12 points) + 1 (beta / s) + (A - 1) (squarings) + 2^A - 1 (butterflies) + 2^A - 1 - A (their constants) = 2 (2^A - 1) + 1.
#pragma once
#include "common.cuh"

namespace zk {

constexpr uint32_t kFriMaxArityLog = 3;
constexpr uint32_t kFriTableLoBits = 12;   // the two-level power table: lo[i] = w^-i (i < 2^12), hi[i] = w^-(i << 12)

struct FriConsts {
    Mul29 c;                                      // beta / s
    Mul29 w[(1 << (kFriMaxArityLog - 1)) - 1];    // w_{2^A}^-(j + 1), j + 1 < 2^(A-1)
};
struct FriTable {
    const uint64_t *lo;    // 2^lo_bits elements w^-i, w = root_of_unity(2^log_domain)
    const uint64_t *hi;    // 2^(log_domain - lo_bits) elements w^-(i << lo_bits)
    uint32_t lo_bits;      // min(log_domain, kFriTableLoBits)
    uint32_t hi_bits;      // log_domain - lo_bits: 0 = the low table alone
    uint32_t stride_log;   // the layer's root is w^(2^stride_log): output i takes exponent i << stride_log
};

// (the two non-template kernels here are static: mlbatch.hip includes this header beside fri.hip, for the butterfly)
// both levels of the power table of w^-1: thread t < 2^lo_bits the low entry, the next 2^hi_bits threads the high entries
static __global__ __launch_bounds__(kBlock) void k_fri_tables(uint64_t *__restrict__ lo, uint64_t *__restrict__ hi, uint32_t lo_bits, uint32_t hi_bits,
                                                       Fe winv, FieldParams P) {
    const uint64_t n_lo = 1ull << lo_bits, total = n_lo + (1ull << hi_bits), stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const bool low = t < n_lo;
        Fe acc = fe_one(P), b = winv;   // square and multiply
        for (uint64_t e = low ? t : (t - n_lo) << lo_bits; e; e >>= 1) {
            if (e & 1) acc = fe_mul(acc, b, P);
            b = fe_mul(b, b, P);
        }
        fe_store(low ? lo : hi, low ? t : t - n_lo, acc);
    }
}

// w_N^-i for output i (the high table only where the domain has one: tw.hi_bits is wave-uniform)
ZK_D Fe fri_twiddle(const FriTable &tw, uint64_t i, const FieldParams &P) {
    const uint64_t e = i << tw.stride_log;
    const Fe lo = fe_load(tw.lo, e & ((1ull << tw.lo_bits) - 1));
    if (tw.hi_bits == 0) return lo;
    return fe_mul_tt(lo, fe_load(tw.hi, e >> tw.lo_bits), P);
}
// a / 2: the Montgomery form of a / 2 is half the Montgomery form of a, and an odd representative becomes even by adding p (< 2^255: no
// carry out of the eight limbs)
ZK_D Fe fe_half(const Fe &a, const FieldParams &P) {
    const uint32_t mask = 0u - (a.v[0] & 1u);
    uint32_t pm[8], t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pm[i] = P.p[i] & mask;
    add8(t, a.v, pm);
    Fe r;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.v[i] = (t[i] >> 1) | (t[i + 1] << 31);
    r.v[7] = t[7] >> 1;
    return r;
}
// the A butterfly levels over the 2^A inputs of one output; u = U_L
// (level L and butterfly J as template parameters: every index into the argument struct and into x is a constant, so neither goes to
// scratch)
template <int A, int L, int J>
ZK_D void fri_butterfly(Fe (&x)[1 << A], const Fe &u, const FriConsts &kc, const FieldParams &P) {
    constexpr int h = 1 << (A - 1 - L);
    Fe d = fe_sub(x[J], x[J + h], P);
    if constexpr (J > 0) d = fe_mul29(d, kc.w[(J << L) - 1], P);   // w_{2^A}^(-2^L J)
    x[J] = fe_add(fe_add(x[J], x[J + h], P), fe_mul_tt(d, u, P), P);
    if constexpr (J + 1 < h) fri_butterfly<A, L, J + 1>(x, u, kc, P);
}
template <int A, int L>
ZK_D void fri_level(Fe (&x)[1 << A], const Fe &u, const FriConsts &kc, const FieldParams &P) {
    fri_butterfly<A, L, 0>(x, u, kc, P);
    if constexpr (L + 1 < A) fri_level<A, L + 1>(x, fe_mul_tt(u, u, P), kc, P);
}
template <int A>
ZK_D Fe fri_butterflies(Fe (&x)[1 << A], const Fe &t /* w_N^-i */, const FriConsts &kc, const FieldParams &P) {
    fri_level<A, 0>(x, fe_mul29(t, kc.c, P), kc, P);
    Fe o = x[0];
#pragma unroll
    for (int l = 0; l < A; ++l) o = fe_half(o, P);
    return o;
}

// out[i], i < M = 2^(n - A), from in[i + j M], j < 2^A.  RUN: M is a multiple of 64; a wave moves 64 consecutive elements of each of the
// 2^A input streams and of the output as two coalesced 1-KiB dwordx4 accesses, nontemporal, exactly as k_fold_msb does (lane l ends up
// owning element pair_owned(l) of the run).  !RUN (M < 64): one 32-byte element per lane.  Out of place only.
template <int A, bool RUN>
__global__ __launch_bounds__(kBlock) void k_fri_fold(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t M, FriTable tw, FriConsts kc,
                                                     FieldParams P) {
    if (RUN) {
        const uint32_t lane = threadIdx.x & 63;
        const bool odd = lane & 1;
        const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
        const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
        const uint4 *in4 = reinterpret_cast<const uint4 *>(in);
        uint4 *out4 = reinterpret_cast<uint4 *>(out);
        for (uint64_t e0 = wave * 64; e0 < M; e0 += nwaves * 64) {
            const uint64_t c0 = 2 * e0 + lane;   // element e occupies uint4 slots 2e, 2e + 1
            Fe x[1 << A];
#pragma unroll
            for (int j = 0; j < (1 << A); ++j) {
                const uint4 a = nt_load16(in4 + c0 + 2 * (uint64_t)j * M), b = nt_load16(in4 + c0 + 2 * (uint64_t)j * M + 64);
                x[j] = pair_gather(a, b, odd);
            }
            const Fe o = fri_butterflies<A>(x, fri_twiddle(tw, e0 + pair_owned(lane), P), kc, P);
            uint4 oa, ob;
            pair_scatter(o, odd, oa, ob);
            nt_store16(oa, out4 + c0);
            nt_store16(ob, out4 + c0 + 64);
        }
    } else {
        const uint64_t stride = (uint64_t)gridDim.x * kBlock;
        for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += stride) {
            Fe x[1 << A];
#pragma unroll
            for (int j = 0; j < (1 << A); ++j) x[j] = fe_load(in, i + (uint64_t)j * M);
            fe_store(out, i, fri_butterflies<A>(x, fri_twiddle(tw, i, P), kc, P));
        }
    }
}

// The openings of one layer for all queries in one launch: for query q with row rho = idx[q] mod M the 2^A row elements layer[rho + j M]
// (Montgomery, as stored) and the log2 M siblings tree_level[d][(rho >> d) ^ 1], bottom up, into the staging block at `rows` / `paths`
// (4 words per item).  `tree` holds the levels as merkle.hip lays them out: level d starts at digest 2^(m+1) - 2^(m-d+1), m = log2 M.
static __global__ __launch_bounds__(kBlock) void k_fri_gather(const uint64_t *__restrict__ layer, const uint64_t *__restrict__ tree, uint32_t log_m, uint32_t arity,
                                                       const uint64_t *__restrict__ idx, uint64_t n_queries, uint64_t *__restrict__ rows,
                                                       uint64_t *__restrict__ paths) {
    const uint32_t per = arity + log_m;
    const uint64_t M = 1ull << log_m, total = n_queries * per, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < total; it += stride) {
        const uint64_t q = it / per, rho = idx[q] & (M - 1);
        const uint32_t r = (uint32_t)(it % per);
        const uint64_t *src;
        uint64_t *dst;
        if (r < arity) {
            src = layer + 4 * (rho + (uint64_t)r * M);
            dst = rows + 4 * (q * arity + r);
        } else {
            const uint32_t d = r - arity;
            src = tree + 4 * (((2ull << log_m) - (2ull << (log_m - d))) + ((rho >> d) ^ 1));
            dst = paths + 4 * (q * log_m + d);
        }
        const uint4 a = reinterpret_cast<const uint4 *>(src)[0], b = reinterpret_cast<const uint4 *>(src)[1];
        reinterpret_cast<uint4 *>(dst)[0] = a;
        reinterpret_cast<uint4 *>(dst)[1] = b;
    }
}

}  // namespace zk
