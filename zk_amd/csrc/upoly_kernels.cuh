// upoly_kernels.cuh -- UnivariatePolynomial (polynomial/src/univariate_poly.rs) on the device: the direct product for small
// operands and the evaluation sum.  The NTT product runs on the fused variants of k_ntt_pass (ntt_kernels.cuh); the host side
// is capi.hip's zk_upoly_* section, the design DESIGN.md section 11.
#pragma once
#include "common.cuh"
#include "ntt_kernels.cuh"

namespace zk {

// a * b for canonical a, b on the carry-free core, left in [0, 2p): fe_mul_tt without its final conditional subtraction
ZK_D Fe fe_mul_tt_lazy(const Fe &a, const Fe &b, const FieldParams &P) {
    uint32_t x[9], y[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    Mul29 c;
    split29_shl5(a.v, x);
    split29(b.v, c.l);
    return mul29_core<true, false>(x, y, c, P);
}

// Direct product (Mul for &UnivariatePolynomial, univariate_poly.rs:186-209, restated per output coefficient):
// out[k] = sum_j s[j] * l[k - j] over max(0, k - ll + 1) <= j <= min(k, ls - 1), s the shorter operand.  One thread per
// output; the threads of a wave read the same s[j] (a broadcast) and consecutive l[k - j].  The sum is kept in [0, 2p) like the
// NTT's values and reduced once.  Exact field arithmetic: bit-identical to the reference's double loop.
__global__ __launch_bounds__(kBlock) void k_upoly_direct(const uint64_t *__restrict__ s, uint64_t ls, const uint64_t *__restrict__ l,
                                                         uint64_t ll, uint64_t *__restrict__ out, FieldParams P) {
    const uint64_t lc = ls + ll - 1, stride = (uint64_t)gridDim.x * kBlock;
    const Mod2p M2 = mod2p_of(P);
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < lc; k += stride) {
        const uint64_t j0 = k + 1 > ll ? k + 1 - ll : 0, j1 = k < ls - 1 ? k : ls - 1;
        Fe acc = fe_zero();
        for (uint64_t j = j0; j <= j1; ++j) acc = fe_add2(acc, fe_mul_tt_lazy(fe_load(s, j), fe_load(l, k - j), P), M2);
        fe_store(out, k, fe_canon2(acc, P));
    }
}

// Power table of x in the NTT twiddles' two-level form (k_ntt_tables): lo[i] = prepared x^i, i < 2^lo_bits, and
// hi[h] = prepared x^(h << lo_bits), h < n_hi -- both Mul29 records (x^e * 2^5, nine 29-bit limbs), so x^i * c costs one
// fe_mul29.  Every entry by its own square-and-multiply (at most 2^12 + n_hi entries of <= 40 squarings).
__global__ __launch_bounds__(kBlock) void k_upoly_powers(uint32_t *__restrict__ lo, uint32_t *__restrict__ hi, uint32_t lo_bits,
                                                         uint64_t n_hi, Fe x, FieldParams P) {
    const uint64_t n_lo = 1ull << lo_bits, total = n_lo + n_hi, stride = (uint64_t)gridDim.x * kBlock;
    Fe x_hi = x;   // x^(2^lo_bits)
    for (uint32_t i = 0; i < lo_bits; ++i) x_hi = fe_sqr(x_hi, P);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += stride) {
        const bool is_hi = idx >= n_lo;
        uint64_t e = is_hi ? idx - n_lo : idx;
        Fe base = is_hi ? x_hi : x, acc = fe_one(P);
        while (e) {
            if (e & 1) acc = fe_mul(acc, base, P);
            base = fe_sqr(base, P);
            e >>= 1;
        }
        store_mul29((is_hi ? hi + (idx - n_lo) * kTw29Words : lo + idx * kTw29Words), mul29_prepare(acc, P));
    }
}

// canonical sum of the block's values in LDS (kBlock elements of [0, 2p)), returned to thread 0
ZK_D Fe upoly_block_sum(Fe v, Fe *red, const FieldParams &P) {
    const Mod2p M2 = mod2p_of(P);
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t h = kBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] = fe_add2(red[threadIdx.x], red[threadIdx.x + h], M2);
        __syncthreads();
    }
    return fe_canon2(red[0], P);
}

// UnivariatePolynomial::evaluate (univariate_poly.rs:29-40, Horner) as a sum: sum_i c[i] x^i = sum_h x^(h 2^lo) (sum_l c[h 2^lo + l] x^l).
// Block b takes the chunks h = b, b + grid, ...; thread t the terms l = t, t + kBlock, ... of a chunk: one multiplication by lo[l]
// per coefficient, one by hi[h] per chunk and thread.  Partial sums in [0, 2p), one canonical partial per block.
__global__ __launch_bounds__(kBlock) void k_upoly_eval(const uint64_t *__restrict__ c, uint64_t len, const uint32_t *__restrict__ lo,
                                                       const uint32_t *__restrict__ hi, uint32_t lo_bits, FieldParams P,
                                                       uint64_t *__restrict__ partials) {
    __shared__ Fe red[kBlock];
    const Mod2p M2 = mod2p_of(P);
    const uint64_t chunk = 1ull << lo_bits, n_hi = (len + chunk - 1) >> lo_bits;
    Fe acc = fe_zero();
    for (uint64_t h = blockIdx.x; h < n_hi; h += gridDim.x) {
        const uint64_t base = h << lo_bits;
        Fe part = fe_zero();
        for (uint64_t i = threadIdx.x; i < chunk && base + i < len; i += kBlock)
            part = fe_add2(part, fe_mul29_t<true>(fe_load(c, base + i), load_mul29(lo + i * kTw29Words), P), M2);
        acc = fe_add2(acc, fe_mul29_t<true>(part, load_mul29(hi + h * kTw29Words), P), M2);
    }
    const Fe s = upoly_block_sum(acc, red, P);
    if (threadIdx.x == 0) fe_store(partials, blockIdx.x, s);
}
// second stage: one block sums the partials of k_upoly_eval
__global__ __launch_bounds__(kBlock) void k_upoly_eval_final(const uint64_t *__restrict__ partials, uint32_t n, FieldParams P,
                                                             uint64_t *__restrict__ out) {
    __shared__ Fe red[kBlock];
    const Mod2p M2 = mod2p_of(P);
    Fe acc = fe_zero();
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) acc = fe_add2(acc, fe_load(partials, i), M2);
    const Fe s = upoly_block_sum(acc, red, P);
    if (threadIdx.x == 0) fe_store(out, 0, s);
}

}  // namespace zk
