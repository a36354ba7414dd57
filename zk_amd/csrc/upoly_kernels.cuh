// upoly_kernels.cuh -- UnivariatePolynomial (polynomial/src/univariate_poly.rs) on the device: the direct product for small
// operands, the evaluation sum, Add, and the weights, direct tree levels and block merges of the interpolation.  The NTT product
// and the NTT tree levels run on the fused variants of k_ntt_pass (ntt_kernels.cuh); the host side is ntt.hip's zk_upoly_*
// section, the design DESIGN.md section 11.
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


// Add for &UnivariatePolynomial (univariate_poly.rs:157-184): out[k] = a[k] + b[k] over max(la, lb) coefficients, a missing
// coefficient counting as 0 -- which is also the reference's copy of the other operand when one of them is empty.
__global__ __launch_bounds__(kBlock) void k_upoly_add(const uint64_t *__restrict__ a, uint64_t la, const uint64_t *__restrict__ b,
                                                      uint64_t lb, uint64_t *__restrict__ out, FieldParams P) {
    const uint64_t n = la > lb ? la : lb, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride)
        fe_store(out, k, fe_add(k < la ? fe_load(a, k) : fe_zero(), k < lb ? fe_load(b, k) : fe_zero(), P));
}

// ---- interpolation (UnivariatePolynomial::interpolate / ::interpolate_xy, univariate_poly.rs:43-80) -------------
// F::from(i as u64)
ZK_D Fe fe_from_index(uint64_t i, const FieldParams &P) {
    Fe v = {{(uint32_t)i, (uint32_t)(i >> 32), 0, 0, 0, 0, 0, 0}};
    return fe_from_canonical(v, P);
}
// a^(p-2) (Fermat; 0 -> 0), square and multiply over the bits of p - 2
ZK_D Fe fe_inverse_dev(const Fe &a, const FieldParams &P) {
    uint32_t e[8], two[8] = {2, 0, 0, 0, 0, 0, 0, 0};
    sub8(e, P.p, two);
    Fe acc = fe_one(P);
    for (int i = (int)P.bits - 1; i >= 0; --i) {
        acc = fe_mul_tt(acc, acc, P);
        if ((e[i >> 5] >> (i & 31)) & 1u) acc = fe_mul_tt(acc, a, P);
    }
    return acc;
}

// Exclusive product scans over n values, forward (out[i] = prod_{k < i} v[k]) or backward (out[i] = prod_{k > i} v[k]); v null:
// v[k] = F::from(max(k, 1)), the factors of the factorials.  Three launches: per-chunk products, one block scanning them (and the
// grand total at totals[n_chunks]), and the chunks again with their prefixes.  Exact: a product's bits do not depend on its order.
constexpr uint32_t kScanPerThread = 16, kScanChunk = kBlock * kScanPerThread;
ZK_D Fe scan_value(const uint64_t *v, uint64_t k, const FieldParams &P) { return v ? fe_load(v, k) : fe_from_index(k ? k : 1, P); }
// exclusive product scan of the block's thread values (kBlock of them) in LDS; returns thread t's prefix, *total the block's product
ZK_D Fe block_scan_excl(Fe x, Fe *red, const FieldParams &P, Fe *total) {
    const uint32_t t = threadIdx.x;
    red[t] = x;
    __syncthreads();
    for (uint32_t h = 1; h < kBlock; h <<= 1) {   // Hillis-Steele, inclusive
        const Fe y = t >= h ? fe_mul_tt(red[t - h], red[t], P) : red[t];
        __syncthreads();
        red[t] = y;
        __syncthreads();
    }
    const Fe r = t ? red[t - 1] : fe_one(P);
    *total = red[kBlock - 1];
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(kBlock) void k_scan_prod_partial(const uint64_t *__restrict__ v, uint64_t n, int rev, FieldParams P,
                                                              uint64_t *__restrict__ totals) {
    __shared__ Fe red[kBlock];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kScanPerThread;
    Fe acc = fe_one(P);
    for (uint32_t q = 0; q < kScanPerThread && i0 + q < n; ++q) acc = fe_mul_tt(acc, scan_value(v, rev ? n - 1 - (i0 + q) : i0 + q, P), P);
    Fe total;
    (void)block_scan_excl(acc, red, P, &total);
    if (threadIdx.x == 0) fe_store(totals, blockIdx.x, total);
}
// one block: totals[0..nc) -> exclusive prefixes, totals[nc] = the product of all
__global__ __launch_bounds__(kBlock) void k_scan_prod_totals(uint64_t *__restrict__ totals, uint32_t nc, FieldParams P) {
    __shared__ Fe red[kBlock];
    const uint32_t per = (nc + kBlock - 1) / kBlock, j0 = threadIdx.x * per;
    Fe acc = fe_one(P);
    for (uint32_t q = 0; q < per && j0 + q < nc; ++q) acc = fe_mul_tt(acc, fe_load(totals, j0 + q), P);
    Fe total;
    Fe pre = block_scan_excl(acc, red, P, &total);
    for (uint32_t q = 0; q < per && j0 + q < nc; ++q) {
        const Fe x = fe_load(totals, j0 + q);
        fe_store(totals, j0 + q, pre);
        pre = fe_mul_tt(pre, x, P);
    }
    if (threadIdx.x == 0) fe_store(totals, nc, total);
}
__global__ __launch_bounds__(kBlock) void k_scan_prod_apply(const uint64_t *__restrict__ v, uint64_t n, int rev, FieldParams P,
                                                            const uint64_t *__restrict__ totals, uint64_t *__restrict__ out) {
    __shared__ Fe red[kBlock];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kScanPerThread;
    Fe acc = fe_one(P);
    for (uint32_t q = 0; q < kScanPerThread && i0 + q < n; ++q) acc = fe_mul_tt(acc, scan_value(v, rev ? n - 1 - (i0 + q) : i0 + q, P), P);
    Fe total;
    Fe pre = fe_mul_tt(fe_load(totals, blockIdx.x), block_scan_excl(acc, red, P, &total), P);
    for (uint32_t q = 0; q < kScanPerThread && i0 + q < n; ++q) {
        const uint64_t k = rev ? n - 1 - (i0 + q) : i0 + q;
        const Fe x = scan_value(v, k, P);
        fe_store(out, k, pre);
        pre = fe_mul_tt(pre, x, P);
    }
}
// one thread: *out = (*in)^-1
__global__ void k_fe_invert_one(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, FieldParams P) {
    if (threadIdx.x == 0 && blockIdx.x == 0) fe_store(out, 0, fe_inverse_dev(fe_load(in, 0), P));
}

// interpolate (xs = 0 .. n-1): w_i = y_i / prod_{j != i} (i - j) = y_i (-1)^(n-1-i) / (i! (n-1-i)!), with 1/i! = suf[i] / (n-1)!,
// suf[i] = prod_{i < k < n} k (the backward scan) and inv_tot = 1/(n-1)!
__global__ __launch_bounds__(kBlock) void k_interp_weights_index(const uint64_t *__restrict__ ys, const uint64_t *__restrict__ suf,
                                                                 const uint64_t *__restrict__ inv_tot, uint64_t n, FieldParams P,
                                                                 uint64_t *__restrict__ w) {
    const Fe it = fe_load(inv_tot, 0), it2 = fe_mul_tt(it, it, P);
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        Fe v = fe_mul_tt(fe_mul_tt(fe_load(ys, i), it2, P), fe_mul_tt(fe_load(suf, i), fe_load(suf, n - 1 - i), P), P);
        if ((n - 1 - i) & 1) v = fe_neg(v, P);
        fe_store(w, i, v);
    }
}
// interpolate_xy: d_i = prod_{j != i, j < nx} (x_i - x_j) for i < m, 1 for m <= i < nx.  One lane per i, xs in LDS tiles of kBlock;
// *flag = 1 if some d_i (i < m) is 0 -- a repeated x the reference's (x_i - x_j).inverse().unwrap() panics on (:68)
__global__ __launch_bounds__(kBlock) void k_interp_denoms(const uint64_t *__restrict__ xs, uint64_t nx, uint64_t m, FieldParams P,
                                                          uint64_t *__restrict__ d, uint32_t *__restrict__ flag) {
    __shared__ Fe tile[kBlock];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if ((uint64_t)blockIdx.x * kBlock >= m) {   // (block-uniform) no weight here
        if (i < nx) fe_store(d, i, fe_one(P));
        return;
    }
    const bool act = i < m;
    const Fe xi = act ? fe_load(xs, i) : fe_zero();
    Fe acc = fe_one(P);
    for (uint64_t j0 = 0; j0 < nx; j0 += kBlock) {
        if (j0 + threadIdx.x < nx) tile[threadIdx.x] = fe_load(xs, j0 + threadIdx.x);
        __syncthreads();
        const uint32_t cnt = nx - j0 < kBlock ? (uint32_t)(nx - j0) : kBlock;
        if (act) {
            for (uint32_t q = 0; q < cnt; ++q)
                if (j0 + q != i) acc = fe_mul_tt(acc, fe_sub(xi, tile[q], P), P);
        }
        __syncthreads();
    }
    if (i < nx) fe_store(d, i, act ? acc : fe_one(P));
    if (act && fe_is_zero(acc)) atomicOr(flag, 1u);
}
// interpolate_xy: w_i = y_i * pre[i] * suf[i] / prod_k d_k = y_i / d_i for i < m, 0 above
__global__ __launch_bounds__(kBlock) void k_interp_weights_xy(const uint64_t *__restrict__ ys, const uint64_t *__restrict__ pre,
                                                              const uint64_t *__restrict__ suf, const uint64_t *__restrict__ inv_tot,
                                                              uint64_t n, uint64_t m, FieldParams P, uint64_t *__restrict__ w) {
    const Fe it = fe_load(inv_tot, 0);
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        fe_store(w, i, i < m ? fe_mul_tt(fe_mul_tt(fe_load(ys, i), it, P), fe_mul_tt(fe_load(pre, i), fe_load(suf, i), P), P) : fe_zero());
}

// Subproduct tree, direct levels.  Node of 2s points over [b, b + 2s): M = x^(2s) + m(x) kept as m's 2s coefficients, and
// P = sum_i w_i M / (x - x_i) (< 2s coefficients), both at [b, b + 2s) of their arrays.  Two siblings L, R of s points combine to
//   m = x^s (m_L + m_R) + m_L m_R,   P = x^s (P_L + P_R) + P_L m_R + P_R m_L.
// Level l (s = 2^l) combines the nodes of the prefix of n with its low l + 1 bits cleared (the complete subtrees; n's binary blocks,
// largest first, start at multiples of their size).  Block c owns points [c 2^D, c 2^D + 2^D) in LDS, one per thread, builds the
// leaves (m = -x_i, P = w_i) and runs levels 0 .. D-1; the chunk past the last multiple of 2^D runs the same rule on its length.
template <int D>
__global__ __launch_bounds__(1 << D) void k_interp_tree_direct(const uint64_t *__restrict__ w, const uint64_t *__restrict__ xs, uint64_t n,
                                                               FieldParams P, uint64_t *__restrict__ mo, uint64_t *__restrict__ po) {
    __shared__ Fe lm[1 << D], lp[1 << D];
    const Mod2p M2 = mod2p_of(P);
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x << D;
    const uint32_t r = n - base < (1u << D) ? (uint32_t)(n - base) : (1u << D);
    if (t < r) {
        lm[t] = fe_neg(xs ? fe_load(xs, base + t) : fe_from_index(base + t, P), P);
        lp[t] = fe_load(w, base + t);
    }
    __syncthreads();
    for (uint32_t l = 0; l < (uint32_t)D; ++l) {
        const uint32_t s = 1u << l, covered = (r >> (l + 1)) << (l + 1);
        if (!covered) break;   // (block-uniform)
        Fe a = fe_zero(), b = fe_zero();
        if (t < covered) {
            const uint32_t nb = t & ~(2 * s - 1), k = t & (2 * s - 1);
            const uint32_t j0 = k >= s ? k - s + 1 : 0, j1 = k < s ? k : s - 1;
            for (uint32_t j = j0; j <= j1; ++j) {
                const Fe mr = lm[nb + s + k - j], ml = lm[nb + k - j];
                a = fe_add2(a, fe_mul_tt_lazy(lm[nb + j], mr, P), M2);
                b = fe_add2(b, fe_mul_tt_lazy(lp[nb + j], mr, P), M2);
                b = fe_add2(b, fe_mul_tt_lazy(lp[nb + s + j], ml, P), M2);
            }
            a = fe_canon2(a, P);
            b = fe_canon2(b, P);
            if (k >= s) {
                a = fe_add(a, fe_add(lm[nb + k - s], lm[nb + k], P), P);
                b = fe_add(b, fe_add(lp[nb + k - s], lp[nb + k], P), P);
            }
        }
        __syncthreads();
        if (t < covered) {
            lm[t] = a;
            lp[t] = b;
        }
        __syncthreads();
    }
    if (t < r) {
        fe_store(mo, base + t, lm[t]);
        fe_store(po, base + t, lp[t]);
    }
}

// Merge of two adjacent blocks A (a points, left) and T (t points, right) whose products are given: mm = m_A m_T, pm = P_A m_T,
// mp = P_T m_A (a + t - 1 coefficients each).  (x^a + m_A)(x^t + m_T) and P_A M_T + P_T M_A give, for k < a + t,
//   m[k] = mm[k] + m_T[k - a] + m_A[k - t],   P[k] = pm[k] + mp[k] + P_A[k - t] + P_T[k - a]   (terms with a negative index: 0).
// mo null: m is not needed (the last merge).
__global__ __launch_bounds__(kBlock) void k_interp_merge(const uint64_t *__restrict__ ma, const uint64_t *__restrict__ pa, uint64_t a,
                                                         const uint64_t *__restrict__ mt, const uint64_t *__restrict__ pt, uint64_t t,
                                                         const uint64_t *__restrict__ mm, const uint64_t *__restrict__ pm,
                                                         const uint64_t *__restrict__ mp, FieldParams P, uint64_t *__restrict__ mo,
                                                         uint64_t *__restrict__ po) {
    const uint64_t n = a + t, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        Fe p = k + 1 < n ? fe_add(fe_load(pm, k), fe_load(mp, k), P) : fe_zero();
        if (k >= t) p = fe_add(p, fe_load(pa, k - t), P);
        if (k >= a) p = fe_add(p, fe_load(pt, k - a), P);
        fe_store(po, k, p);
        if (mo) {
            Fe v = k + 1 < n && mm ? fe_load(mm, k) : fe_zero();
            if (k >= a) v = fe_add(v, fe_load(mt, k - a), P);
            if (k >= t) v = fe_add(v, fe_load(ma, k - t), P);
            fe_store(mo, k, v);
        }
    }
}

}  // namespace zk
