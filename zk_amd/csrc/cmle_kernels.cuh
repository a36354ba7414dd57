// cmle_kernels.cuh -- a dense CoeffMultilinearPolynomial (coefficient_form.rs) on the device: 2^n coefficients in KEY order (key
// bit v <-> variable v), next to the evaluation table in hypercube order (table index bit n-1-v <-> variable v).
//
//   interpolate (:200-216)          key-order coefficients = Moebius transform of the table, bit-reversed:  T[x | b] -= T[x]
//   to_evaluation_form (:340-347)   table = zeta transform of the key-order coefficients, bit-reversed:      T[x | b] += T[x]
//
// Both are one transform over every index bit plus a bit reversal of the index, and both run as the zeta passes of
// zeta_kernels.cuh do (LDS tile, its swizzle and register groups), subtracting or adding:
//
//   pass 1  (k_cmle_first):  a workgroup owns the 2^(lo + hi) entries whose index differs in the low `lo` and the high `hi` bits
//            (the middle bits fixed by the workgroup), runs those lo + hi levels in LDS and stores the tile at the bit-reversed
//            indices.  Reversal maps the low bits to the high ones and back, so both sides move runs: reads are 2^lo consecutive
//            entries, writes 2^hi (lo = 5, hi = 6 from 2^11 on: 1 and 2 KiB).  Out of place: the input is left as it was.
//   pass 2+ (k_cmle_tile):   the middle bits, now at output positions [hi, n - lo), at most 8 per pass, in place, as k_zeta_tile
//            does; the run of a tile is 2^min(pos, 11 - L) entries, so a pass may start below bit 11.
//
//   2^24: 11 + 7 + 6 bits, three crossings of the table (1.5 GiB read + 1.5 GiB written).
//
// evaluate (:39-69) reuses the MLE evaluator: (1, r) = (1 + r) (1 - r', r') with r' = r / (1 + r), so sum_k c_k prod_{v in k} r_v is
// prod (1 + r_v) times the multilinear evaluation of the coefficient vector read as a table.  A coordinate r = -1 has no such
// factor; k_cmle_fold_minus_one takes its variable out first (c[k] - c[k | bit v]).  to_bytes (:131-139) is k_cmle_records.
#pragma once
#include "zeta_tile.cuh"

namespace zk {

constexpr uint32_t kCmleFirstLo = 5, kCmleFirstHi = 6;   // pass 1 at 2^11 and up: runs of 32 entries read, 64 written

// zeta_group with the butterfly's sign as a parameter
template <int G, bool kSub>
ZK_D void cmle_group(unsigned char *smem, uint32_t s, uint32_t tile_log, const FieldParams &P) {
    uint4 *plo = reinterpret_cast<uint4 *>(smem), *phi = reinterpret_cast<uint4 *>(smem + kZetaPlaneBytes);
    const uint32_t items = 1u << (tile_log - G);
    for (uint32_t w = threadIdx.x; w < items; w += kBlock) {
        const uint32_t low = w & ((1u << s) - 1u), high = w >> s;
        const uint32_t i0 = (high << (s + G)) | low;
        Fe x[1 << G];
#pragma unroll
        for (int u = 0; u < (1 << G); ++u) {
            const uint32_t sl = zeta_slot(i0 | ((uint32_t)u << s));
            const uint4 a = plo[sl], b = phi[sl];
            x[u] = {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
        }
#pragma unroll
        for (int b = 0; b < G; ++b)
#pragma unroll
            for (int c = 0; c < (1 << G); ++c)
                if (c & (1 << b)) x[c] = kSub ? fe_sub(x[c], x[c ^ (1 << b)], P) : fe_add(x[c], x[c ^ (1 << b)], P);
#pragma unroll
        for (int u = 1; u < (1 << G); ++u) {   // entry 0 of a group never changes
            const uint32_t sl = zeta_slot(i0 | ((uint32_t)u << s));
            plo[sl] = make_uint4(x[u].v[0], x[u].v[1], x[u].v[2], x[u].v[3]);
            phi[sl] = make_uint4(x[u].v[4], x[u].v[5], x[u].v[6], x[u].v[7]);
        }
    }
}
// levels of bits [lb, lb + L) of the tile-local index; ends with the tile complete in LDS (barrier included)
template <bool kSub>
ZK_D void cmle_levels(unsigned char *smem, uint32_t lb, uint32_t L, uint32_t tile_log, const FieldParams &P) {
    for (uint32_t s = lb; s < lb + L;) {
        const uint32_t g = lb + L - s >= 3 ? 3u : lb + L - s;
        __syncthreads();
        if (g == 3) cmle_group<3, kSub>(smem, s, tile_log, P);
        else if (g == 2) cmle_group<2, kSub>(smem, s, tile_log, P);
        else cmle_group<1, kSub>(smem, s, tile_log, P);
        s += g;
    }
    __syncthreads();
}
// the k low bits of x, reversed (k <= 32)
ZK_D uint32_t brev_bits(uint32_t x, uint32_t k) { return k ? __brev(x) >> (32u - k) : 0u; }

// pass 1: in (2^n entries, those at index >= in_len read as zero) -> out at bit-reversed indices, levels of the low `lo` and high `hi`
// index bits done.  gridDim.x = 2^(n - lo - hi): workgroup M owns the input indices (h << (n - hi)) | (M << lo) | l.  Tile-local index
// (h << lo) | l.  Its output index is brev(l) << (n - lo) | brev(M) << hi | brev(h): row brev(l) of 2^lo, column brev(h) of a run of 2^hi.
template <bool kSub>
__global__ __launch_bounds__(kBlock) void k_cmle_first(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t in_len, uint32_t n,
                                                       uint32_t lo, uint32_t hi, FieldParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, tile_log = lo + hi, m = n - tile_log;
    const uint64_t M = blockIdx.x;
    const uint4 *g_in = reinterpret_cast<const uint4 *>(in);
    uint4 *g_out = reinterpret_cast<uint4 *>(out);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (uint32_t q = tid; q < (2u << tile_log); q += kBlock) {   // piece q: half (q & 1) of entry l = (q >> 1) mod 2^lo of row h
        const uint32_t h = q >> (lo + 1), piece = q & ((2u << lo) - 1u);
        const uint64_t j = ((uint64_t)h << (n - hi)) | (M << lo) | (piece >> 1);
        uint4 v = zero;
        if (j < in_len) v = g_in[2 * j + (piece & 1)];
        *reinterpret_cast<uint4 *>(smem + (piece & 1) * kZetaPlaneBytes + zeta_slot((h << lo) | (piece >> 1)) * 16) = v;
    }
    cmle_levels<kSub>(smem, 0, tile_log, tile_log, P);
    const uint64_t mid = (uint64_t)brev_bits((uint32_t)M, m) << hi;
    for (uint32_t q = tid; q < (2u << tile_log); q += kBlock) {   // piece q: half (q & 1) of column (q >> 1) mod 2^hi of output row r
        const uint32_t r = q >> (hi + 1), piece = q & ((2u << hi) - 1u), col = piece >> 1;
        const uint32_t i = (brev_bits(col, hi) << lo) | brev_bits(r, lo);
        g_out[2 * (((uint64_t)r << (n - lo)) | mid | col) + (piece & 1)] =
            *reinterpret_cast<const uint4 *>(smem + (piece & 1) * kZetaPlaneBytes + zeta_slot(i) * 16);
    }
}

// passes 2+: index bits [pos, pos + L), 1 <= L <= 8, in place.  Tile = 2^L rows x C = 2^log_c consecutive entries (log_c <= pos,
// L + log_c <= 11); tile-local index (row << log_c) | col.  One workgroup per tile, gridDim.x = 2^(n - L - log_c).
template <bool kSub>
__global__ __launch_bounds__(kBlock) void k_cmle_tile(uint64_t *table, uint32_t pos, uint32_t L, uint32_t log_c, FieldParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, tile_log = L + log_c;
    const uint64_t outer = (uint64_t)blockIdx.x >> (pos - log_c), cg = (uint64_t)blockIdx.x & ((1ull << (pos - log_c)) - 1);
    const uint64_t base = (outer << (pos + L)) + (cg << log_c);
    uint4 *g4 = reinterpret_cast<uint4 *>(table);
    const uint32_t pieces_log = log_c + 1;   // 16-byte pieces per run
#pragma unroll 4
    for (uint32_t q = tid; q < (2u << tile_log); q += kBlock) {
        const uint32_t row = q >> pieces_log, piece = q & ((1u << pieces_log) - 1u);
        const uint4 v = g4[2 * (base + ((uint64_t)row << pos)) + piece];
        const uint32_t i = (row << log_c) | (piece >> 1);
        *reinterpret_cast<uint4 *>(smem + (piece & 1) * kZetaPlaneBytes + zeta_slot(i) * 16) = v;
    }
    cmle_levels<kSub>(smem, log_c, L, tile_log, P);
#pragma unroll 4
    for (uint32_t q = tid; q < (2u << tile_log); q += kBlock) {
        const uint32_t row = q >> pieces_log, piece = q & ((1u << pieces_log) - 1u);
        if (row == 0) continue;   // row 0 of a tile never changes
        const uint32_t i = (row << log_c) | (piece >> 1);
        g4[2 * (base + ((uint64_t)row << pos)) + piece] =
            *reinterpret_cast<const uint4 *>(smem + (piece & 1) * kZetaPlaneBytes + zeta_slot(i) * 16);
    }
}

// the variable of key bit v assigned -1: out[k] = in[k] - in[k | 2^v] over the n_out = 2^(n-1) keys without bit v
__global__ __launch_bounds__(kBlock) void k_cmle_fold_minus_one(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t n_out,
                                                                uint32_t v, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, low_mask = (1ull << v) - 1;
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < n_out; o += stride) {
        const uint64_t k = ((o & ~low_mask) << 1) | (o & low_mask);
        fe_store(out, o, fe_sub(fe_load(in, k), fe_load(in, k | (1ull << v)), P));
    }
}

// ---- algebra on the present keys (partial_evaluate :72-104, relabel :109-123, scalar_multiply :272-282, Add :350-373, Mul :375-415) ----
// A handle that has been partially evaluated holds the keys {k : k & fixed == 0}, ascending, as a compact vector of 2^m entries
// (m = n_vars - popcount(fixed)): compact index j <-> key pdep(j, ~fixed).  All kernels below work on compact indices.

// the low bits of x scattered to the set bits of mask, lowest first (pdep); popcount(mask) steps
ZK_D uint64_t cmle_pdep(uint64_t x, uint64_t mask) {
    uint64_t r = 0;
    for (uint64_t bit = 1; mask; bit <<= 1) {
        const uint64_t low = mask & (0 - mask);
        if (x & bit) r |= low;
        mask ^= low;
    }
    return r;
}

// partial_evaluate of up to three variables in one pass.  q[0] < q[1] < q[2] are their bit positions in the compact index of `in`; w[T]
// is the product of the assigned values of the variables whose bit is set in T (bit i of T <-> q[i]; w[0] = 1 is never read).  One
// thread per output o:   out[o] = sum_T w[T] * in[base | spread(T)],   base = o with a zero bit inserted at each q[i].
// Field arithmetic is exact and fully reduced, so the sum equals the reference's one-variable-at-a-time multiply-and-add in any order.
//
// Grouping (host, cmle_contract_passes): the assigned positions are taken from the HIGHEST down, three per pass, so every pass but the
// last contracts three (the first reads the source once and writes 1/8 of it: at most 1 + 1/7 of the source is read in total), the
// remainder of one or two is the last and smallest pass, and the low positions -- whose load instructions coalesce worst -- end up
// together in the cheapest pass.  Positions not yet contracted lie below those that are, so they keep their numbers between passes.
struct CmleContract {
    Fe w[8];
    uint32_t q[3];
};
template <int G>
ZK_D uint64_t cmle_insert_zeros(uint64_t o, const uint32_t *q) {
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const uint64_t low = (1ull << q[i]) - 1;
        o = ((o & ~low) << 1) | (o & low);
    }
    return o;
}
// The 2^G operands come straight from global memory: a position >= 3 gives each load instruction runs of >= 256 B; with positions 0..2
// each lane reads its own 64-256 B run, every fetched line is used, but a load instruction touches up to 64 lines.
template <int G>
__global__ __launch_bounds__(kBlock) void k_cmle_contract(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t n_out,
                                                           CmleContract g, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < n_out; o += stride) {
        const uint64_t base = cmle_insert_zeros<G>(o, g.q);
        Fe x[1 << G];
#pragma unroll
        for (int t = 0; t < (1 << G); ++t) {
            uint64_t k = base;
#pragma unroll
            for (int i = 0; i < G; ++i)
                if (t >> i & 1) k |= 1ull << g.q[i];
            x[t] = fe_load(in, k);
        }
        Fe acc = x[0];
#pragma unroll
        for (int t = 1; t < (1 << G); ++t) acc = fe_add(acc, fe_mul(x[t], g.w[t], P), P);
        fe_store(out, o, acc);
    }
}

// scalar_multiply (:272-282): out[j] = in[j] * s over the n present keys
__global__ __launch_bounds__(kBlock) void k_cmle_scale(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t n, Fe s, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) fe_store(out, j, fe_mul(fe_load(in, j), s, P));
}
// Add (:350-373): the longer operand's n_long keys, the shorter one's n_short <= n_long summed into the low keys
__global__ __launch_bounds__(kBlock) void k_cmle_add(const uint64_t *__restrict__ longer, uint64_t n_long, const uint64_t *__restrict__ shorter,
                                                      uint64_t n_short, uint64_t *__restrict__ out, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n_long; j += stride) {
        Fe x = fe_load(longer, j);
        if (j < n_short) x = fe_add(x, fe_load(shorter, j), P);
        fe_store(out, j, x);
    }
}
// Mul (:375-415): the lhs variables come first, out[i | j << n_a] = a[i] * b[j] over 2^(n_a + n_b) outputs.  Consecutive threads take
// consecutive i (a run of a, 32-byte stores side by side); b[j] is the same for 2^n_a outputs in a row.  n_a = 0 or n_b = 0 is the
// reference's scalar path (:380-384) with the scalar read from the device.
__global__ __launch_bounds__(kBlock) void k_cmle_outer(const uint64_t *__restrict__ a, uint32_t n_a, const uint64_t *__restrict__ b,
                                                        uint64_t n_out, uint64_t *__restrict__ out, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, mask_a = (1ull << n_a) - 1;
    for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < n_out; o += stride)
        fe_store(out, o, fe_mul(fe_load(a, o & mask_a), fe_load(b, o >> n_a), P));
}

// to_bytes records (coefficient_form.rs:131-139) of keys first_key .. first_key + n - 1: the key as 8 bytes big-endian (usize), then
// the canonical coefficient as 32 bytes big-endian (into_bigint().to_bytes_be()); 40 bytes each, written as five 8-byte words.  On a
// partially evaluated handle (present != 0: the mask of the variables still present) first_key counts compact indices and the record's
// key is pdep(index, present), which ascends with the index as the BTreeMap's keys do.
__global__ __launch_bounds__(kBlock) void k_cmle_records(const uint64_t *__restrict__ in, uint8_t *__restrict__ out, uint64_t first_key,
                                                         uint64_t n, FieldParams P, uint64_t present = 0) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
        const Fe c = fe_to_canonical(fe_load(in, j), P);
        const uint64_t key = present ? cmle_pdep(first_key + j, present) : first_key + j;
        uint2 *o = reinterpret_cast<uint2 *>(out + 40 * j);
        o[0] = make_uint2(__builtin_bswap32((uint32_t)(key >> 32)), __builtin_bswap32((uint32_t)key));
        o[1] = make_uint2(__builtin_bswap32(c.v[7]), __builtin_bswap32(c.v[6]));
        o[2] = make_uint2(__builtin_bswap32(c.v[5]), __builtin_bswap32(c.v[4]));
        o[3] = make_uint2(__builtin_bswap32(c.v[3]), __builtin_bswap32(c.v[2]));
        o[4] = make_uint2(__builtin_bswap32(c.v[1]), __builtin_bswap32(c.v[0]));
    }
}

}  // namespace zk
