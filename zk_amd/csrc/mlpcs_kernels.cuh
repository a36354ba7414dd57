// mlpcs_kernels.cuh -- gfx950 kernels of the multilinear polynomial commitment (no reference item; definition: tests/mlpcs_ref.py; host
// side: mlpcs.hip): the sumcheck of t(x) eq(x, z) without an eq table.
//
// Round r of the opening needs, of T_r (2^(m+1) elements, variable 0 = the top index bit), the two sums
//   S_X = sum_{x' < 2^m} T_r[X 2^m + x'] W(x'),   W(x') = eq(x', (z_{r+1} .. z_{n-1})),   X = 0, 1
// (the host makes h_r(0), h_r(1), h_r(2) of them).  W is a tensor product, so it is read as Hi[x' >> L] Lo[x' & (2^L - 1)], L = min(m,
// kMlLoBits): Lo over the last L variables sits in LDS, Hi over the m - L variables before them in memory.  A wave takes a run of 2^S
// consecutive x' that share one Hi entry (S = L where the table is large; down to 6 where 2^(m-L) runs would leave most of the device
// idle: 2^(m-S) runs, about 2^kMlRunsTargetLog at least): per lane the products T Lo are added up over the run's 2^(S-6) trips, the two
// sums are multiplied by Hi once, and the lanes are added up once, at the end of the kernel -- one multiplication per table element and
// 2 / 2^(S-6) more.
// A prefix slice of a larger eq table is no Hi: the scale it carries, prod (1 - z_j) over the variables left out, is zero when a z_j is 1.
// So k_ml_eq_tables makes every suffix's own tables: the Hi table of k variables at hi[2^k ..], the Lo table of k variables at lo[2^k ..]
// (entry [1] is the table of no variable, the constant one): fewer than 2^(n-L) + 2^(L+1) elements in all.
//
// FOLD: the launch of round r >= 1 reads T_{r-1} once as four coalesced streams (x' + j 2^m, j < 4: the access pattern of
// k_fri_fold<2>), folds at beta_{r-1} (T_r[i] = T_{r-1}[i] + beta (T_{r-1}[i + 2^(m+1)] - T_{r-1}[i])), writes T_r once and sums it on the
// way.  !FOLD (round 0, zk_mle_eq_sums): two streams, nothing written.  RUN: m >= 6, a wave moves 64-element runs as k_fold_msb does;
// !RUN: one workgroup, one x' per thread, Lo alone (m < 6 <= kMlLoBits).  Per-workgroup partials [block][2] go to k_round_tail (ns = 2).
#pragma once
#include "common.cuh"

namespace zk {

constexpr uint32_t kMlLoBits = 9;       // the Lo table: 2^9 elements = 16 KiB of LDS, runs of 512 elements (8 trips of a wave)
constexpr uint32_t kMlRunMinBits = 6;   // m >= 6: the run kernel
constexpr uint32_t kMlRunsTargetLog = 11;   // a run is 2^S elements, S = min(L, max(6, m - 11)): 2048 runs where the table has them

// every suffix's Hi and Lo table of the variables vars[0 .. nvars): lo_max = min(nvars, kMlLoBits), hi_max = nvars - lo_max.
// lo[2^k + j], k <= lo_max: eq(j, the last k variables); hi[2^k + j], k <= hi_max: eq(j, the k variables before the last lo_max).
// One thread per entry, k dependent multiplications.  (static, as the other non-template kernels that two units include: mlpcs.hip, mlbatch.hip)
static __global__ __launch_bounds__(kBlock) void k_ml_eq_tables(const uint64_t *__restrict__ vars, uint32_t nvars, uint32_t lo_max, uint64_t *__restrict__ hi,
                                                         uint64_t *__restrict__ lo, FieldParams P) {
    const uint32_t hi_max = nvars - lo_max;
    const uint64_t n_hi = 2ull << hi_max, total = n_hi + (2ull << lo_max), stride = (uint64_t)gridDim.x * kBlock;
    const Fe one = fe_one(P);
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const bool is_hi = t < n_hi;
        const uint64_t e = is_hi ? t : t - n_hi;
        if (e == 0) continue;   // entry 0 of either block belongs to no table
        const uint32_t k = 63u - (uint32_t)__builtin_clzll(e);
        const uint64_t j = e - (1ull << k);
        const uint32_t first = (is_hi ? hi_max : nvars) - k;   // the table's first variable
        Fe acc = one;
        for (uint32_t w = 0; w < k; ++w) {
            const Fe g = fe_load(vars, first + w);
            acc = fe_mul(acc, (j >> (k - 1 - w)) & 1 ? g : fe_sub(one, g, P), P);
        }
        fe_store(is_hi ? hi : lo, e, acc);
    }
}

// src: T_{r-1} (FOLD: 2^(m+2) elements) or T_r itself (!FOLD: 2^(m+1)); dst: T_r (FOLD only); hi / lo: this round's tables (2^(m-L)
// and 2^L entries, L = min(m, kMlLoBits)); S (RUN only, 6 <= S <= L): log2 of a run; partials: [gridDim.x][2]
template <bool FOLD, bool RUN>
__global__ __launch_bounds__(kBlock) void k_ml_round(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, uint32_t m, uint32_t S, const uint64_t *__restrict__ hi,
                                                     const uint64_t *__restrict__ lo, Mul29 beta, uint64_t *__restrict__ partials, FieldParams P) {
    __shared__ __attribute__((aligned(16))) uint64_t lo_s[RUN ? (4u << kMlLoBits) : 4];
    __shared__ Fe wave_sums[2 * (kBlock / 64)];
    const uint64_t half = 1ull << m;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Fe tot0 = fe_zero(), tot1 = fe_zero();
    if (RUN) {
        const uint32_t L = m < kMlLoBits ? m : kMlLoBits;
        for (uint32_t i = threadIdx.x; i < (1u << L); i += kBlock) fe_store(lo_s, i, fe_load(lo, i));
        __syncthreads();
        const bool odd = lane & 1;
        const uint32_t own = pair_owned(lane), trips = 1u << (S - 6), lo_mask = (1u << L) - 1;
        const uint64_t n_runs = half >> S;
        const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + wv, nwaves = (uint64_t)gridDim.x * (kBlock / 64);
        const uint4 *in4 = reinterpret_cast<const uint4 *>(src);
        uint4 *out4 = reinterpret_cast<uint4 *>(dst);
        for (uint64_t run = wave; run < n_runs; run += nwaves) {
            Fe acc0 = fe_zero(), acc1 = fe_zero();
            for (uint32_t t = 0; t < trips; ++t) {
                const uint64_t e0 = (run << S) + 64 * t;   // the first x' of this trip
                const uint64_t c0 = 2 * e0 + lane;         // element e occupies uint4 slots 2e, 2e + 1
                Fe x0, x1;
                if (FOLD) {
                    Fe v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint4 a = nt_load16(in4 + c0 + 2 * (uint64_t)j * half), b = nt_load16(in4 + c0 + 2 * (uint64_t)j * half + 64);
                        v[j] = pair_gather(a, b, odd);
                    }
                    x0 = fe_sub(v[0], fe_mul29(fe_sub(v[0], v[2], P), beta, P), P);
                    x1 = fe_sub(v[1], fe_mul29(fe_sub(v[1], v[3], P), beta, P), P);
                    uint4 oa, ob;
                    pair_scatter(x0, odd, oa, ob);   // plain stores: the next round reads T_r again
                    out4[c0] = oa;
                    out4[c0 + 64] = ob;
                    pair_scatter(x1, odd, oa, ob);
                    out4[c0 + 2 * half] = oa;
                    out4[c0 + 2 * half + 64] = ob;
                } else {
                    x0 = pair_gather(in4[c0], in4[c0 + 64], odd);
                    x1 = pair_gather(in4[c0 + 2 * half], in4[c0 + 2 * half + 64], odd);
                }
                const Fe w = fe_load(lo_s, ((uint32_t)e0 & lo_mask) + own);
                acc0 = fe_add(acc0, fe_mul_tt(x0, w, P), P);
                acc1 = fe_add(acc1, fe_mul_tt(x1, w, P), P);
            }
            const Fe h = fe_load(hi, run >> (L - S));   // wave-uniform address
            tot0 = fe_add(tot0, fe_mul_tt(acc0, h, P), P);
            tot1 = fe_add(tot1, fe_mul_tt(acc1, h, P), P);
        }
    } else {
        if (threadIdx.x < half) {   // one workgroup; m < 6: Lo is the whole W, read from memory
            const uint64_t i = threadIdx.x;
            Fe x0, x1;
            if (FOLD) {
                const Fe a0 = fe_load(src, i), a1 = fe_load(src, i + half), a2 = fe_load(src, i + 2 * half), a3 = fe_load(src, i + 3 * half);
                x0 = fe_sub(a0, fe_mul29(fe_sub(a0, a2, P), beta, P), P);
                x1 = fe_sub(a1, fe_mul29(fe_sub(a1, a3, P), beta, P), P);
                fe_store(dst, i, x0);
                fe_store(dst, i + half, x1);
            } else {
                x0 = fe_load(src, i);
                x1 = fe_load(src, i + half);
            }
            const Fe w = fe_load(lo, i);
            tot0 = fe_mul_tt(x0, w, P);
            tot1 = fe_mul_tt(x1, w, P);
        }
    }
    tot0 = fe_wave_sum(tot0, P);
    tot1 = fe_wave_sum(tot1, P);
    if (lane == 0) {
        wave_sums[2 * wv] = tot0;
        wave_sums[2 * wv + 1] = tot1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        Fe s = wave_sums[threadIdx.x];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) s = fe_add(s, wave_sums[2 * w + threadIdx.x], P);
        fe_store(partials, 2 * (uint64_t)blockIdx.x + threadIdx.x, s);
    }
}

}  // namespace zk
