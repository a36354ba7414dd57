// pcs_kernels.cuh -- gfx950 kernels of the FRI polynomial commitment (no reference item; definition: tests/pcs_ref.py; host side: pcs.hip;
// DESIGN.md section 15).  The hot path is the DEEP quotient over the extension domain,
//   q[i] = (sum_c alpha^c (F_c[i] - y_c)) / (x_i - z),   x_i = s w^i,  i < N = 2^n,
// as Montgomery's trick in the batch inversion's shape (inv_kernels.cuh) with the denominators GENERATED, not loaded: the k columns are
// read once, q is written once, and neither x_i - z nor its inverse ever reaches HBM.
//   launch 1  k_pcs_chunk_products   per chunk of 2^11 outputs the product of its denominators (x_i from a two-level power table)
//   launch 2  k_pcs_totals           one workgroup: the inverses of the chunk products, with the call's ONE fe_inverse_binary
//   launch 3  k_pcs_apply            regenerates the chunk's denominators, walks the product tree down and, in the same pass, forms the
//                                    numerator by Horner over the columns and multiplies
// and one launch of k_pcs_apply<ALONE> at or below one chunk.  sum_c alpha^c (F_c[i] - y_c) = (sum_c alpha^c F_c[i]) - Y with
// Y = sum_c alpha^c y_c, which the host forms once (exact arithmetic: the same canonical element), so the kernel carries one constant
// for all y_c, whatever k is.  z, Y and alpha (prepared, Mul29) are kernel arguments: wave-uniform, SGPRs.  k is a run-time loop over
// a device array of column pointers (uniform index: scalar loads).
// Multiplications per output above one chunk and above 2^12 points: launch 1: 1 (power table compose) + 1 (chunk product); launch 3:
// 1 (compose) + 1 (prefix) + 2 (back-substitution) + k - 1 (Horner, by the prepared alpha) + 1 (numerator times inverse); the two LDS
// trees add 3 * 255 / 2048 < 0.4 per launch-3 output and 255 / 2048 per launch-1 output: k + 6 and about 0.5.  Up to 2^12 points the
// low table alone holds x_i (no compose): k + 4.  One more per output in the TIMES_X form, which writes x_i q[i] (what zk_pcs_open hands to FRI).
#pragma once
#include "common.cuh"
#include "inv_field.cuh"
#include "inv_tree.cuh"

namespace zk {

// elements per thread and per workgroup: the batch inversion's (inv_kernels.cuh kInvPerThread, kInvChunk), for the same reason -- 8
// denominators and 8 prefixes stay in registers without scratch (profiles/pcs_resource_usage.md); tests/pcs_ref.py QUOTIENT_LOGS
// straddles kPcsChunk and the table split
constexpr uint32_t kPcsPerThread = 8;
constexpr uint32_t kPcsChunk = kBlock * kPcsPerThread;
constexpr uint32_t kPcsTableLoBits = 12;   // the two-level power table: lo[i] = s w^i (i < 2^12), hi[i] = w^(i << 12)
constexpr uint32_t kPcsPtrBatch = 32;

struct PcsTable {
    const uint64_t *lo;   // 2^lo_bits elements s w^i, w = root_of_unity(2^n)
    const uint64_t *hi;   // 2^hi_bits elements w^(i << lo_bits)
    uint32_t lo_bits;     // min(n, kPcsTableLoBits)
    uint32_t hi_bits;     // n - lo_bits: 0 = the low table alone
};
struct PcsConsts {
    Fe z;          // the opening point
    Fe y;          // Y = sum_c alpha^c y_c
    Mul29 alpha;   // prepared: the Horner multiplier
};
struct PcsPtrs {
    const uint64_t *p[kPcsPtrBatch];
};

// table[base + j] = b.p[j]: the column pointers reach device memory as launch arguments (no host copy to wait for)
__global__ void k_pcs_put_ptrs(const uint64_t **table, uint32_t base, uint32_t count, PcsPtrs b) {
    if (threadIdx.x < count) table[base + threadIdx.x] = b.p[threadIdx.x];
}
// both levels of the power table: thread t < 2^lo_bits the low entry s w^t, the next 2^hi_bits threads the high entries
__global__ __launch_bounds__(kBlock) void k_pcs_tables(uint64_t *__restrict__ lo, uint64_t *__restrict__ hi, uint32_t lo_bits, uint32_t hi_bits, Fe w, Fe s,
                                                       FieldParams P) {
    const uint64_t n_lo = 1ull << lo_bits, total = n_lo + (1ull << hi_bits), stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const bool low = t < n_lo;
        Fe acc = low ? s : fe_one(P), b = w;   // square and multiply
        for (uint64_t e = low ? t : (t - n_lo) << lo_bits; e; e >>= 1) {
            if (e & 1) acc = fe_mul(acc, b, P);
            b = fe_mul(b, b, P);
        }
        fe_store(low ? lo : hi, low ? t : t - n_lo, acc);
    }
}
// x_i - z (never zero: the host refuses a z on the domain); the high table only where the domain has one (tb.hi_bits is uniform)
ZK_D Fe pcs_den(const PcsTable &tb, uint64_t i, const Fe &z, const FieldParams &P) {
    const Fe lo = fe_load(tb.lo, i & ((1ull << tb.lo_bits) - 1));
    if (tb.hi_bits == 0) return fe_sub(lo, z, P);
    return fe_sub(fe_mul_tt(lo, fe_load(tb.hi, i >> tb.lo_bits), P), z, P);
}

// launch 1 of 3: totals[c] = the product of chunk c's denominators.  Which thread takes which element of the chunk does not matter
// for a product: thread t takes base + q kBlock + t, so a wave reads 64 consecutive entries of the low table.
__global__ __launch_bounds__(kBlock) void k_pcs_chunk_products(uint64_t n, PcsTable tb, Fe z, FieldParams P, uint64_t *__restrict__ totals) {
    __shared__ Fe node[2 * kBlock];
    const uint64_t base = (uint64_t)blockIdx.x * kPcsChunk + threadIdx.x;
    const Fe one = fe_one(P);
    Fe acc = one;
#pragma unroll
    for (uint32_t q = 0; q < kPcsPerThread; ++q) {
        const uint64_t i = base + (uint64_t)q * kBlock;
        const Fe x = i < n ? pcs_den(tb, i, z, P) : one;
        acc = q ? fe_mul_tt(acc, x, P) : x;
    }
    inv_tree_up(acc, node, P);
    if (threadIdx.x == 0) fe_store(totals, blockIdx.x, node[1]);
}
// launch 2 of 3, one workgroup: inv[c] = 1 / totals[c] for the nc chunk products -- the same trick one level up, thread t taking the
// run of `per` consecutive chunks from t * per, with the call's only field inversion (k_inv_totals without its zero counts: no
// denominator is zero here).  inv[] holds the run's prefixes in between.
__global__ __launch_bounds__(kBlock) void k_pcs_totals(const uint64_t *__restrict__ totals, uint64_t nc, FieldParams P, uint64_t *__restrict__ inv) {
    __shared__ Fe node[2 * kBlock];
    const uint64_t per = (nc + kBlock - 1) / kBlock, j0 = threadIdx.x * per < nc ? threadIdx.x * per : nc, j1 = j0 + per < nc ? j0 + per : nc;
    Fe acc = fe_one(P);
    for (uint64_t j = j0; j < j1; ++j) {
        fe_store(inv, j, acc);
        acc = fe_mul_tt(acc, fe_load(totals, j), P);
    }
    inv_tree_up(acc, node, P);
    if (threadIdx.x == 0) node[1] = fe_inverse_binary(node[1], P);
    Fe back = inv_tree_down(node, P);
    for (uint64_t j = j1; j-- > j0;) {
        fe_store(inv, j, fe_mul_tt(back, fe_load(inv, j), P));
        back = fe_mul_tt(back, fe_load(totals, j), P);
    }
}

// one column value / one output of the element a lane owns.  RUN (n a multiple of 64): `i0` is the first element of the wave's run of
// 64, moved as two coalesced 1-KiB dwordx4 accesses, nontemporal, as k_fri_fold moves its streams (the lane ends up owning element
// i0 + pair_owned(lane)); !RUN (n < 64): `i0` is the lane's own element.
template <bool RUN>
ZK_D Fe pcs_load(const uint64_t *col, uint64_t i0, uint32_t lane) {
    if (RUN) return run_load_nt(col + 4 * i0, lane);
    return fe_load(col, i0);
}
template <bool RUN>
ZK_D void pcs_store(uint64_t *out, uint64_t i0, uint32_t lane, const Fe &e) {
    if (RUN) run_store_nt(out + 4 * i0, lane, e);
    else fe_store(out, i0, e);
}
// launch 3 of 3 (ALONE = false): out[i] over chunk blockIdx.x given inv[blockIdx.x] = the inverse of the product of its denominators;
// ALONE = true is the whole call in one launch for n <= kPcsChunk: the workgroup inverts its product itself.  TIMES_X: out[i] is
// x_i q[i], the evaluations of X q(X).  Out of place only.
template <bool ALONE, bool RUN, bool TIMES_X>
__global__ __launch_bounds__(kBlock) void k_pcs_apply(const uint64_t *const *__restrict__ cols, uint32_t k, uint64_t n, PcsTable tb, PcsConsts kc,
                                                      FieldParams P, const uint64_t *__restrict__ inv, uint64_t *__restrict__ out) {
    __shared__ Fe node[2 * kBlock];
    const uint32_t lane = threadIdx.x & 63;
    // q = 0: the wave's run (RUN) or the lane's element; q advances both by kBlock
    const uint64_t first = (uint64_t)blockIdx.x * kPcsChunk + (RUN ? (threadIdx.x & ~63u) : threadIdx.x);
    const uint32_t own = RUN ? pair_owned(lane) : 0;
    const Fe one = fe_one(P);
    Fe x[kPcsPerThread], pre[kPcsPerThread];   // pre[q] = x[0] ... x[q-1]
    Fe acc = one;
    inv_static_for<0, kPcsPerThread>([&](auto qc) {
        constexpr uint32_t q = decltype(qc)::value;
        const uint64_t i0 = first + (uint64_t)q * kBlock;
        x[q] = i0 < n ? pcs_den(tb, i0 + own, kc.z, P) : one;   // (n is a multiple of 64 under RUN: a run is inside or outside as a whole)
        pre[q] = acc;
        acc = q ? fe_mul_tt(acc, x[q], P) : x[q];
    });
    inv_tree_up(acc, node, P);
    if (threadIdx.x == 0) node[1] = ALONE ? fe_inverse_binary(node[1], P) : fe_load(inv, blockIdx.x);
    Fe back = inv_tree_down(node, P);   // the inverse of x[0] ... x[kPcsPerThread - 1]
    inv_static_for<0, kPcsPerThread>([&](auto qc) {
        constexpr uint32_t q = kPcsPerThread - 1 - decltype(qc)::value;
        const uint64_t i0 = first + (uint64_t)q * kBlock;
        Fe o = q ? fe_mul_tt(back, pre[q], P) : back;   // 1 / x[q]
        if (TIMES_X) o = fe_add(fe_mul_tt(o, kc.z, P), one, P);   // x_i / (x_i - z) = 1 + z / (x_i - z): x[q] need not outlive the line below
        if (q) back = fe_mul_tt(back, x[q], P);
        if (i0 < n) {   // wave-uniform under RUN
            // Horner over the columns, two per trip so that both loads are in flight before the first multiplication
            uint32_t c = k - 1;
            Fe num = pcs_load<RUN>(cols[c], i0, lane);
            for (; c >= 2; c -= 2) {
                const Fe f1 = pcs_load<RUN>(cols[c - 1], i0, lane), f0 = pcs_load<RUN>(cols[c - 2], i0, lane);
                num = fe_add(fe_mul29(fe_add(fe_mul29(num, kc.alpha, P), f1, P), kc.alpha, P), f0, P);
            }
            if (c) num = fe_add(fe_mul29(num, kc.alpha, P), pcs_load<RUN>(cols[0], i0, lane), P);
            pcs_store<RUN>(out, i0, lane, fe_mul_tt(fe_sub(num, kc.y, P), o, P));
        }
    });
}

// ---- the k values y_c = f_c(z) of one opening: coefficients c of polynomial blockIdx.y at coeffs + 4 (blockIdx.y << log_len) (zero
// padded to 2^log_len).  A thread runs Horner over kPcsEvalRun consecutive coefficients and scales by z^(first index); the workgroup
// adds up.  Two launches for all k, so that the values come back with one download.
constexpr uint32_t kPcsEvalRun = 16, kPcsEvalMaxBlocks = 64;
ZK_D Fe pcs_block_sum(Fe v, Fe *red, const FieldParams &P) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t h = kBlock / 2; h >= 1; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] = fe_add(red[threadIdx.x], red[threadIdx.x + h], P);
        __syncthreads();
    }
    return red[0];
}
__global__ __launch_bounds__(kBlock) void k_pcs_eval_partial(const uint64_t *__restrict__ coeffs, uint32_t log_len, Fe z, FieldParams P,
                                                             uint64_t *__restrict__ partials) {
    __shared__ Fe red[kBlock];
    const uint64_t len = 1ull << log_len, n_runs = (len + kPcsEvalRun - 1) / kPcsEvalRun, stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t *co = coeffs + 4 * ((uint64_t)blockIdx.y << log_len);
    Fe sum = fe_zero();
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n_runs; r += stride) {
        const uint64_t j0 = r * kPcsEvalRun, j1 = j0 + kPcsEvalRun < len ? j0 + kPcsEvalRun : len;
        Fe acc = fe_load(co, j1 - 1);
        for (uint64_t j = j1 - 1; j-- > j0;) acc = fe_add(fe_mul_tt(acc, z, P), fe_load(co, j), P);
        Fe pw = fe_one(P), b = z;   // z^j0
        for (uint64_t e = j0; e; e >>= 1) {
            if (e & 1) pw = fe_mul_tt(pw, b, P);
            b = fe_mul_tt(b, b, P);
        }
        sum = fe_add(sum, fe_mul_tt(acc, pw, P), P);
    }
    sum = pcs_block_sum(sum, red, P);
    if (threadIdx.x == 0) fe_store(partials, (uint64_t)blockIdx.y * gridDim.x + blockIdx.x, sum);
}
__global__ __launch_bounds__(kBlock) void k_pcs_eval_final(const uint64_t *__restrict__ partials, uint32_t per_poly, FieldParams P,
                                                           uint64_t *__restrict__ values) {
    __shared__ Fe red[kBlock];
    Fe sum = fe_zero();
    for (uint32_t j = threadIdx.x; j < per_poly; j += kBlock) sum = fe_add(sum, fe_load(partials, (uint64_t)blockIdx.x * per_poly + j), P);
    sum = pcs_block_sum(sum, red, P);
    if (threadIdx.x == 0) fe_store(values, blockIdx.x, sum);
}

}  // namespace zk
