// upoly_kernels.cuh -- UnivariatePolynomial (polynomial/src/univariate_poly.rs) on the device: the direct product for small
// operands, the evaluation sum, Add, the weights, direct tree levels and block merges of the interpolation, the multipoint
// evaluation's direct kernel and the small kernels of its transposed tree, and the division's direct kernel, linear-divisor scan and
// glue.  The NTT product
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
// (block_scan_excl, the block's exclusive LDS product scan, is in common.cuh: inv_kernels.cuh's running products share it)
ZK_D Fe scan_value(const uint64_t *v, uint64_t k, const FieldParams &P) { return v ? fe_load(v, k) : fe_from_index(k ? k : 1, P); }
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
// the same with the check the reference's .inverse().unwrap() makes: *flag = 1 for *in = 0 (*out is then 0)
__global__ void k_fe_invert_checked(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, FieldParams P, uint32_t *__restrict__ flag) {
    if (threadIdx.x || blockIdx.x) return;
    const Fe v = fe_load(in, 0);
    if (fe_is_zero(v)) atomicOr(flag, 1u);
    fe_store(out, 0, fe_inverse_dev(v, P));
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
// MONLY: only m is built (w and po are not touched): the up-sweep of the multipoint evaluation.
template <int D, bool MONLY = false>
__global__ __launch_bounds__(1 << D) void k_interp_tree_direct(const uint64_t *__restrict__ w, const uint64_t *__restrict__ xs, uint64_t n,
                                                               FieldParams P, uint64_t *__restrict__ mo, uint64_t *__restrict__ po) {
    __shared__ Fe lm[1 << D], lp[MONLY ? 1 : 1 << D];
    const Mod2p M2 = mod2p_of(P);
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x << D;
    const uint32_t r = n - base < (1u << D) ? (uint32_t)(n - base) : (1u << D);
    if (t < r) {
        lm[t] = fe_neg(xs ? fe_load(xs, base + t) : fe_from_index(base + t, P), P);
        if constexpr (!MONLY) lp[t] = fe_load(w, base + t);
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
                if constexpr (!MONLY) {
                    b = fe_add2(b, fe_mul_tt_lazy(lp[nb + j], mr, P), M2);
                    b = fe_add2(b, fe_mul_tt_lazy(lp[nb + s + j], ml, P), M2);
                }
            }
            a = fe_canon2(a, P);
            if constexpr (!MONLY) b = fe_canon2(b, P);
            if (k >= s) {
                a = fe_add(a, fe_add(lm[nb + k - s], lm[nb + k], P), P);
                if constexpr (!MONLY) b = fe_add(b, fe_add(lp[nb + k - s], lp[nb + k], P), P);
            }
        }
        __syncthreads();
        if (t < covered) {
            lm[t] = a;
            if constexpr (!MONLY) lp[t] = b;
        }
        __syncthreads();
    }
    if (t < r) {
        fe_store(mo, base + t, lm[t]);
        if constexpr (!MONLY) fe_store(po, base + t, lp[t]);
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

// ---- multipoint evaluation (zk_upoly_evaluate_many: out[i] = p.evaluate(xs[i]), univariate_poly.rs:29-40) --------
// Direct path, O(n L).  Block (bx, by) takes the points [bx kBlock, bx kBlock + kBlock), one per lane, and the coefficients
// [by chunk, by chunk + chunk): the chunk goes through LDS in tiles of kBlock from the top, every lane reads the same LDS word
// (a broadcast, no bank conflict) and runs Horner, acc = acc x + c, with x prepared once as a Mul29.  The block's partial is
// x^start Horner(chunk), at partials[by n + i]; with one chunk that is the result itself.  The second grid axis fills the device when
// the points are few and the polynomial long.  Exact field arithmetic: the same bits as the reference's Horner fold.
__global__ __launch_bounds__(kBlock) void k_evalmany_direct(const uint64_t *__restrict__ c, uint64_t len, const uint64_t *__restrict__ xs,
                                                            uint64_t n, uint64_t chunk, FieldParams P, uint64_t *__restrict__ partials) {
    __shared__ Fe tile[kBlock];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t start = (uint64_t)blockIdx.y * chunk, end = len - start < chunk ? len : start + chunk;
    const bool act = i < n;
    const Fe x = act ? fe_load(xs, i) : fe_zero();
    const Mul29 xp = mul29_prepare(x, P);
    Fe acc = fe_zero();
    for (uint64_t hi = end; hi > start;) {
        const uint64_t lo = hi - start > kBlock ? hi - kBlock : start;
        const uint32_t cnt = (uint32_t)(hi - lo);
        if (threadIdx.x < cnt) tile[threadIdx.x] = fe_load(c, lo + threadIdx.x);
        __syncthreads();
        if (act) {
            for (uint32_t q = cnt; q-- > 0;) acc = fe_add(fe_mul29(acc, xp, P), tile[q], P);
        }
        __syncthreads();
        hi = lo;
    }
    if (!act) return;
    if (start) {   // x^start, square and multiply (block-uniform exponent)
        Fe base = x, pw = fe_one(P);
        for (uint64_t e = start; e; e >>= 1) {
            if (e & 1) pw = fe_mul_tt(pw, base, P);
            base = fe_mul_tt(base, base, P);
        }
        acc = fe_mul_tt(acc, pw, P);
    }
    fe_store(partials, (uint64_t)blockIdx.y * n + i, acc);
}
// second stage: out[i] = sum over the chunks of partials[ch n + i]
__global__ __launch_bounds__(kBlock) void k_evalmany_sum(const uint64_t *__restrict__ partials, uint64_t n, uint32_t chunks, FieldParams P,
                                                         uint64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        Fe acc = fe_load(partials, i);
        for (uint32_t ch = 1; ch < chunks; ++ch) acc = fe_add(acc, fe_load(partials, (uint64_t)ch * n + i), P);
        fe_store(out, i, acc);
    }
}

// Tree path, O(N log^2 N), N = 2^ceil(log2 max(n, L)): the transposed subproduct tree (Bostan, Lecerf, Schost: "Tellegen's principle
// into practice", ISSAC 2003), no polynomial division.  With R(z) = prod_i (1 - x_i z) = rev(M), alpha = 1/R mod z^N and
// b_j = sum_{k >= j} alpha_{k-j} c_k, the value p(x_i) is sum_j b_j q_j for q = R / (1 - x_i z); a node of 2s points holding b hands
// child L the vector b_L[j] = b[j] + cyc_2s(b, m_R)[s + j] and child R the same with m_L (j < s), m the node polynomials of the
// interpolation's up-sweep (every level kept: (log2 N - 7) N 32 bytes).  The levels run on k_ntt_pass's kNttBatch* variants, the
// series inversion and the product for b on the univariate product; the small kernels around them are below.
// out[i] = v[i] for i < n, 0 up to count (the points / nothing padded to N)
__global__ __launch_bounds__(kBlock) void k_evalmany_pad(const uint64_t *__restrict__ v, uint64_t n, uint64_t count, uint64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) fe_store(out, i, i < n ? fe_load(v, i) : fe_zero());
}
// out[i] = F::one(), i < count
__global__ __launch_bounds__(kBlock) void k_fe_fill_one(uint64_t *__restrict__ out, uint64_t count, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) fe_store(out, i, fe_one(P));
}
// R mod z^N from the root's m (M = x^N + m): R_0 = 1, R_k = m[N - k]
__global__ __launch_bounds__(kBlock) void k_evalmany_series(const uint64_t *__restrict__ m, uint64_t N, FieldParams P, uint64_t *__restrict__ R) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < N; k += stride) fe_store(R, k, k ? fe_load(m, N - k) : fe_one(P));
}
// Newton step's middle: g = 2 - e mod z^count, e holding elen >= 1 coefficients (the ones beyond them count as 0)
__global__ __launch_bounds__(kBlock) void k_evalmany_two_minus(const uint64_t *__restrict__ e, uint64_t elen, uint64_t count, FieldParams P,
                                                               uint64_t *__restrict__ g) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const Fe two = fe_add(fe_one(P), fe_one(P), P);
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += stride)
        fe_store(g, k, k ? (k < elen ? fe_neg(fe_load(e, k), P) : fe_zero()) : fe_sub(two, fe_load(e, 0), P));
}
// out[i] = v[N - 1 - i] for N - 1 - i < len, 0 otherwise (i < N): rev(c) padded to N, and b from the product's first N coefficients
__global__ __launch_bounds__(kBlock) void k_evalmany_reverse(const uint64_t *__restrict__ v, uint64_t len, uint64_t N, uint64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += stride)
        fe_store(out, i, N - 1 - i < len ? fe_load(v, N - 1 - i) : fe_zero());
}
// Bottom of the down-sweep: one workgroup per node of s <= 2^7 points, b and the node's R_k = M[s - k] (R_0 = 1) in LDS, one lane per
// point: out_i = sum_{k < s} b_k q_k with q_0 = 1, q_k = R_k + x_i q_{k-1} -- two multiplications a step, every LDS read a broadcast.
// Points at i >= n are the padding: not stored.
constexpr uint32_t kEvalManyBottomLog = 7;
__global__ __launch_bounds__(1 << kEvalManyBottomLog) void k_evalmany_bottom(const uint64_t *__restrict__ b, const uint64_t *__restrict__ m,
                                                                             const uint64_t *__restrict__ xs, uint32_t s, uint64_t n,
                                                                             FieldParams P, uint64_t *__restrict__ out) {
    __shared__ Fe lb[1 << kEvalManyBottomLog], lr[1 << kEvalManyBottomLog];
    const Mod2p M2 = mod2p_of(P);
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * s, i = base + t;
    if (t < s) {
        lb[t] = fe_load(b, base + t);
        lr[t] = t ? fe_load(m, base + s - t) : fe_one(P);
    }
    __syncthreads();
    if (t >= s || i >= n) return;
    const Mul29 xp = mul29_prepare(fe_load(xs, i), P);
    Fe q = fe_one(P), acc = lb[0];
    for (uint32_t k = 1; k < s; ++k) {
        q = fe_add(lr[k], fe_mul29(q, xp, P), P);
        acc = fe_add2(acc, fe_mul_tt_lazy(lb[k], q, P), M2);
    }
    fe_store(out, i, fe_canon2(acc, P));
}
// interpolate_xy's weights from d_i = M'(x_i) (the tree path): 1 at i >= m as k_interp_denoms leaves it, *flag = 1 for a zero d_i, i < m
__global__ __launch_bounds__(kBlock) void k_interp_denoms_fix(uint64_t *__restrict__ d, uint64_t nx, uint64_t m, FieldParams P,
                                                              uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nx; i += stride) {
        if (i >= m) fe_store(d, i, fe_one(P));
        else if (fe_is_zero(fe_load(d, i))) atomicOr(flag, 1u);
    }
}

// ---- division with remainder (zk_upoly_divrem; the reference has none: tests/divrem_ref.py is the definition) -------
// Lengths fix every shape: a (la coefficients) = q b + r with k = la - lb + 1 coefficients of q and lb - 1 of r, nothing trimmed; the
// leading coefficient b[lb - 1] is inverted, and a zero there raises *flag (ZK_ERR_PANIC_INVERSE).
// Newton path's glue: out[i] = v[len - 1 - i], i < count <= len -- rev(v) mod z^count
__global__ __launch_bounds__(kBlock) void k_upoly_reverse_top(const uint64_t *__restrict__ v, uint64_t len, uint64_t count, uint64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) fe_store(out, i, fe_load(v, len - 1 - i));
}
// r[i] = a[i] - qb[i], i < m: the remainder from the low m coefficients of q b
__global__ __launch_bounds__(kBlock) void k_upoly_sub_trunc(const uint64_t *__restrict__ a, const uint64_t *__restrict__ qb, uint64_t m, FieldParams P,
                                                            uint64_t *__restrict__ r) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) fe_store(r, i, fe_sub(fe_load(a, i), fe_load(qb, i), P));
}
// Direct path, la <= kDivremDirectMax: ONE workgroup runs schoolbook long division with the running remainder in LDS (la elements of
// dynamic shared memory, 64 KiB at most).  Lane t keeps b[t], b[t + kBlock], .. in registers.  Step j = k-1 .. 0: every lane forms
// q_j = rem[j + lb - 1] / b_lead from the same LDS word (a broadcast) and prepares it once as a Mul29, the lanes apply
// rem[j + i] -= q_j b[i] (i < lb - 1), one barrier.  The step reads only rem[j + lb - 1], which no lane writes in it.  q null: only
// the positions a later quotient digit reads are kept up to date; r null: not stored.  lb = 1 is a scaling, one lane per coefficient.
constexpr uint32_t kDivremDirectMax = 2048, kDivremRegs = kDivremDirectMax / kBlock;
__global__ __launch_bounds__(kBlock) void k_upoly_divrem_direct(const uint64_t *__restrict__ a, uint32_t la, const uint64_t *__restrict__ b,
                                                                uint32_t lb, FieldParams P, uint64_t *__restrict__ q, uint64_t *__restrict__ r,
                                                                uint32_t *__restrict__ flag) {
    extern __shared__ __align__(16) unsigned char divrem_lds[];
    Fe *rem = reinterpret_cast<Fe *>(divrem_lds);
    const uint32_t t = threadIdx.x, k = la - lb + 1, m = lb - 1;
    const Fe lead = fe_load(b, m);
    if (fe_is_zero(lead)) {   // (block-uniform)
        if (t == 0) atomicOr(flag, 1u);
        return;
    }
    const Fe inv = fe_inverse_dev(lead, P);
    if (m == 0) {
        if (q)
            for (uint32_t j = t; j < k; j += kBlock) fe_store(q, j, fe_mul_tt(fe_load(a, j), inv, P));
        return;
    }
    // (eight named registers and a row macro: an indexed array of them went to scratch)
    static_assert(kDivremRegs == 8, "one register row per kBlock coefficients of b");
    auto row = [&](uint32_t s) { return t + s * kBlock < m ? fe_load(b, t + s * kBlock) : fe_zero(); };
    const Fe b0 = row(0), b1 = row(1), b2 = row(2), b3 = row(3), b4 = row(4), b5 = row(5), b6 = row(6), b7 = row(7);
    for (uint32_t i = t; i < la; i += kBlock) rem[i] = fe_load(a, i);
    __syncthreads();
    const Mul29 invp = mul29_prepare(inv, P);
#define ZK_DIVREM_ROW(s, bs)                                                                         \
    if ((s) * kBlock < m) {                                                                          \
        const uint32_t i = t + (s) * kBlock;                                                         \
        if (i < m && i >= lo) rem[j + i] = fe_sub(rem[j + i], fe_mul29(bs, qp, P), P);               \
    }
    for (uint32_t j = k; j-- > 0;) {
        const Fe qj = fe_mul29(rem[j + m], invp, P);
        const Mul29 qp = mul29_prepare(qj, P);
        if (t == 0 && q) fe_store(q, j, qj);
        const uint32_t lo = r ? 0 : (m > j ? m - j : 0);
        ZK_DIVREM_ROW(0, b0) ZK_DIVREM_ROW(1, b1) ZK_DIVREM_ROW(2, b2) ZK_DIVREM_ROW(3, b3)
        ZK_DIVREM_ROW(4, b4) ZK_DIVREM_ROW(5, b5) ZK_DIVREM_ROW(6, b6) ZK_DIVREM_ROW(7, b7)
        __syncthreads();
    }
#undef ZK_DIVREM_ROW
    if (r)
        for (uint32_t i = t; i < m; i += kBlock) fe_store(r, i, rem[i]);
}
// Linear divisor b = b0 + b1 x, any la >= 2: with inv = 1/b1, z = -b0 inv and S[i] = sum_{t >= i} a[t] z^(t - i) (S[i] = a[i] + z S[i+1])
// the quotient is q[j] = inv S[j + 1] and the remainder r[0] = S[0] = a(z).  A backward scan of that affine recurrence in the three
// phases of k_scan_prod_*: per chunk of kScanChunk coefficients the Horner total H_c = sum_t a[c chunk + t] z^t, one block turning
// the totals into carries S[(c + 1) chunk] = carry_c = carry_(c+1) z^chunk + H_(c+1) (0 for the top chunk; coefficients past la
// count as 0, so a short top chunk needs nothing else) and leaving S[0] behind them, and the chunks again, seeded with their
// carry, storing q.  In a chunk lane t owns the run [16 t, 16 t + 16) and the lanes combine through LDS.
// consts: inv, z, z^16, z^chunk; *flag = 1 for b1 = 0
__global__ void k_divlin_setup(const uint64_t *__restrict__ b, FieldParams P, uint64_t *__restrict__ consts, uint32_t *__restrict__ flag) {
    if (threadIdx.x || blockIdx.x) return;
    const Fe lead = fe_load(b, 1);
    if (fe_is_zero(lead)) atomicOr(flag, 1u);
    const Fe inv = fe_inverse_dev(lead, P);
    Fe pw = fe_neg(fe_mul_tt(fe_load(b, 0), inv, P), P);
    fe_store(consts, 0, inv);
    fe_store(consts, 1, pw);
    for (uint32_t e = 1; e < kScanPerThread; e <<= 1) pw = fe_mul_tt(pw, pw, P);
    fe_store(consts, 2, pw);
    for (uint32_t e = kScanPerThread; e < kScanChunk; e <<= 1) pw = fe_mul_tt(pw, pw, P);
    fe_store(consts, 3, pw);
}
// Horner over the `per` values v[i0 .. i0 + per) below n with the prepared step w: sum_u v[i0 + u] w^u
ZK_D Fe divlin_run(const uint64_t *__restrict__ v, uint64_t n, uint64_t i0, uint32_t per, const Mul29 &wp, const FieldParams &P) {
    Fe acc = fe_zero();
    for (uint32_t u = per; u-- > 0;) {
        acc = fe_mul29(acc, wp, P);
        if (i0 + u < n) acc = fe_add(acc, fe_load(v, i0 + u), P);
    }
    return acc;
}
// the lanes' values h_l, neighbours w apart: leaves red[t] = sum_{l >= t} h_l w^(l - t) (Hillis-Steele from the top, w squared a level)
ZK_D void block_suffix_horner(Fe h, Fe w, Fe *red, const FieldParams &P) {
    const uint32_t t = threadIdx.x;
    red[t] = h;
    __syncthreads();
    for (uint32_t d = 1; d < kBlock; d <<= 1) {
        const Fe y = t + d < kBlock ? fe_add(red[t], fe_mul_tt(red[t + d], w, P), P) : red[t];
        __syncthreads();
        red[t] = y;
        __syncthreads();
        w = fe_mul_tt(w, w, P);
    }
}
__global__ __launch_bounds__(kBlock) void k_divlin_partial(const uint64_t *__restrict__ a, uint64_t la, const uint64_t *__restrict__ consts,
                                                           FieldParams P, uint64_t *__restrict__ totals) {
    __shared__ Fe red[kBlock];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kScanPerThread;
    const Fe h = divlin_run(a, la, i0, kScanPerThread, mul29_prepare(fe_load(consts, 1), P), P);
    block_suffix_horner(h, fe_load(consts, 2), red, P);
    if (threadIdx.x == 0) fe_store(totals, blockIdx.x, red[0]);
}
// one block: totals[0..nc) = H_c -> the carries, totals[nc] = S[0]
__global__ __launch_bounds__(kBlock) void k_divlin_carry(uint64_t *__restrict__ totals, uint32_t nc, const uint64_t *__restrict__ consts, FieldParams P) {
    __shared__ Fe red[kBlock];
    const uint32_t t = threadIdx.x, per = (nc + kBlock - 1) / kBlock, j0 = t * per;
    const Fe Z = fe_load(consts, 3);
    const Mul29 Zp = mul29_prepare(Z, P);
    const Fe g = divlin_run(totals, nc, j0, per, Zp, P);
    Fe base = Z, W = fe_one(P);   // Z^per
    for (uint32_t e = per; e; e >>= 1) {
        if (e & 1) W = fe_mul_tt(W, base, P);
        base = fe_mul_tt(base, base, P);
    }
    block_suffix_horner(g, W, red, P);
    Fe cur = t + 1 < kBlock ? red[t + 1] : fe_zero();
    for (uint32_t u = per; u-- > 0;) {
        if (j0 + u >= nc) continue;
        const Fe H = fe_load(totals, j0 + u);
        fe_store(totals, j0 + u, cur);
        cur = fe_add(fe_mul29(cur, Zp, P), H, P);
    }
    if (t == 0) fe_store(totals, nc, red[0]);
}
__global__ __launch_bounds__(kBlock) void k_divlin_apply(const uint64_t *__restrict__ a, uint64_t la, const uint64_t *__restrict__ consts,
                                                         const uint64_t *__restrict__ carries, FieldParams P, uint64_t *__restrict__ q) {
    __shared__ Fe red[kBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)t * kScanPerThread;
    const Mul29 zp = mul29_prepare(fe_load(consts, 1), P), invp = mul29_prepare(fe_load(consts, 0), P);
    const Fe z16 = fe_load(consts, 2), carry = fe_load(carries, blockIdx.x);
    Fe h = divlin_run(a, la, i0, kScanPerThread, zp, P);
    if (t == kBlock - 1) h = fe_add(h, fe_mul_tt(carry, z16, P), P);   // the carry enters as the coefficient after the chunk
    block_suffix_horner(h, z16, red, P);
    Fe cur = t + 1 < kBlock ? red[t + 1] : carry;   // S[i0 + 16]
    for (uint32_t u = kScanPerThread; u-- > 0;) {
        const uint64_t i = i0 + u;
        if (i >= la) continue;
        cur = fe_add(fe_mul29(cur, zp, P), fe_load(a, i), P);   // S[i]
        if (i) fe_store(q, i - 1, fe_mul29(cur, invp, P));
    }
}

}  // namespace zk
