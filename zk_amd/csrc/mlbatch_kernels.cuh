// mlbatch_kernels.cuh -- gfx950 kernels of the batch multilinear commitment (no reference item; definition: tests/mlbatch_ref.py; host
// side: mlbatch.hip): k tables under one tree, opened at several points by one BaseFold opening of a random linear
// combination.
//
// k_ml_lincomb       out[i] = sum_c coeff[c] src_c[i] over k sources given as a pointer table in device memory: T_0 = sum lambda^c t_c
//                    (and, on the unfused route, the combined layer 0).  A wave moves a run of 64 consecutive elements of every source as
//                    two coalesced 1-KiB dwordx4 loads (common.cuh run_load_nt) and writes the run of `out` once.  The coefficients come
//                    prepared (Mul29, nine words each, made by the host once per launch); they and the pointers have wave-uniform
//                    addresses, so they arrive in SGPRs by scalar loads: one multiplication per source element.
// k_ml_combine_fold  F_1 = fold2(sum_c coeff[c] F_0^c) at beta_0: output i < M reads F_0^c[i] and F_0^c[i + M] of every codeword (2k
//                    streams, the access pattern of k_fri_fold<1>), adds them up into the pair of the virtual layer 0 in registers and
//                    runs fri_kernels.cuh's butterfly on it: the combined layer 0 (2M elements) is never written or read back.
// k_ml_round_many    mlpcs_kernels.cuh's k_ml_round with NP points per pass: NP Lo tables in LDS (16 KiB each at kMlLoBits = 9), NP Hi
//                    entries per run, 2 NP running sums per lane; T is read once (FOLD: T_{r-1} as four streams, T_r written once) whatever
//                    NP is, and every element is multiplied by its NP Lo entries.  NP <= kMlPointsPerPass: 2 NP accumulators and 2 NP
//                    totals of eight registers each are 128 VGPRs at NP = 4 (profiles/mlbatch_resource_usage.md: no instantiation
//                    spills); at 65 KiB of LDS two workgroups share a CU.  Per-workgroup partials [block][2 NP] (slot 2 j + X) go to
//                    k_round_tail.  The Hi / Lo tables of point j are k_ml_eq_tables' of its own tail, hi_stride / lo_stride words apart.
#pragma once
#include <type_traits>

#include "fri_kernels.cuh"
#include "mlpcs_kernels.cuh"

namespace zk {

constexpr uint32_t kMlPointsPerPass = 4;    // tests/mlbatch_ref.py POINTS_PER_PASS
constexpr uint32_t kLincombPerThread = 1;   // elements per thread and trip of k_ml_lincomb's grid-stride loop
constexpr uint32_t kLincombMaxGrid = 16384; // its grid cap: a pure streaming kernel (host_core.hpp kMaxGridStream)

// f(integral constant 0), .. f(N - 1): the per-point loops of k_ml_round_many, unrolled by the template so that every index into the
// per-point register arrays is a constant before the arrays are split (a `#pragma unroll` loop of four left them in scratch)
template <int N, class F>
ZK_D void ml_each(F &&f) {
    if constexpr (N > 0) {
        ml_each<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

template <bool RUN>
__global__ __launch_bounds__(kBlock) void k_ml_lincomb(const uint64_t *const *__restrict__ srcs, uint32_t k, const Mul29 *__restrict__ coef,
                                                       uint64_t *__restrict__ out, uint64_t n_elems, FieldParams P) {
    if (RUN) {   // n_elems is a multiple of 64
        const uint32_t lane = threadIdx.x & 63;
        const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
        for (uint64_t e0 = wave * 64; e0 < n_elems; e0 += nwaves * 64) {
            Fe acc = fe_zero();
#pragma unroll 2
            for (uint32_t c = 0; c < k; ++c) {
                const Mul29 cf = coef[c];
                acc = fe_add(acc, fe_mul29(run_load_nt(srcs[c] + 4 * e0, lane), cf, P), P);
            }
            run_store(out + 4 * e0, lane, acc);   // plain stores: the opening's next launch reads T_0 again
        }
    } else {
        const uint64_t stride = (uint64_t)gridDim.x * kBlock;
        for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_elems; i += stride) {
            Fe acc = fe_zero();
            for (uint32_t c = 0; c < k; ++c) {
                const Mul29 cf = coef[c];
                acc = fe_add(acc, fe_mul29(fe_load(srcs[c], i), cf, P), P);
            }
            fe_store(out, i, acc);
        }
    }
}

// base: codeword c at base + c * stride_words (2M elements each); out: M elements.  RUN: M is a multiple of 64
template <bool RUN>
__global__ __launch_bounds__(kBlock) void k_ml_combine_fold(const uint64_t *__restrict__ base, uint64_t stride_words, uint32_t k, const Mul29 *__restrict__ coef,
                                                            uint64_t *__restrict__ out, uint64_t M, FriTable tw, FriConsts kc, FieldParams P) {
    if (RUN) {
        const uint32_t lane = threadIdx.x & 63;
        const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
        for (uint64_t e0 = wave * 64; e0 < M; e0 += nwaves * 64) {
            Fe x[2] = {fe_zero(), fe_zero()};
#pragma unroll 2
            for (uint32_t c = 0; c < k; ++c) {
                const Mul29 cf = coef[c];
                const uint64_t *cw = base + (uint64_t)c * stride_words + 4 * e0;
                const Fe a0 = run_load_nt(cw, lane), a1 = run_load_nt(cw + 4 * M, lane);
                x[0] = fe_add(x[0], fe_mul29(a0, cf, P), P);
                x[1] = fe_add(x[1], fe_mul29(a1, cf, P), P);
            }
            run_store_nt(out + 4 * e0, lane, fri_butterflies<1>(x, fri_twiddle(tw, e0 + pair_owned(lane), P), kc, P));
        }
    } else {
        const uint64_t stride = (uint64_t)gridDim.x * kBlock;
        for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += stride) {
            Fe x[2] = {fe_zero(), fe_zero()};
            for (uint32_t c = 0; c < k; ++c) {
                const Mul29 cf = coef[c];
                const uint64_t *cw = base + (uint64_t)c * stride_words;
                x[0] = fe_add(x[0], fe_mul29(fe_load(cw, i), cf, P), P);
                x[1] = fe_add(x[1], fe_mul29(fe_load(cw, i + M), cf, P), P);
            }
            fe_store(out, i, fri_butterflies<1>(x, fri_twiddle(tw, i, P), kc, P));
        }
    }
}

// src, dst, m, S, beta: as k_ml_round.  hi / lo: this round's tables of point 0 (2^(m-L) and 2^L entries, L = min(m, kMlLoBits)); point
// j's are hi_stride / lo_stride words further on.  partials: [gridDim.x][2 NP]
template <int NP, bool FOLD, bool RUN>
__global__ __launch_bounds__(kBlock) void k_ml_round_many(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, uint32_t m, uint32_t S,
                                                          const uint64_t *__restrict__ hi, uint64_t hi_stride, const uint64_t *__restrict__ lo, uint64_t lo_stride,
                                                          Mul29 beta, uint64_t *__restrict__ partials, FieldParams P) {
    __shared__ __attribute__((aligned(16))) uint64_t lo_s[RUN ? NP * (4u << kMlLoBits) : 4];
    __shared__ Fe wave_sums[2 * NP * (kBlock / 64)];
    const uint64_t half = 1ull << m;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Fe tot0[NP], tot1[NP];
    ml_each<NP>([&](auto j) { tot0[j] = fe_zero(), tot1[j] = fe_zero(); });
    if (RUN) {
        const uint32_t L = m < kMlLoBits ? m : kMlLoBits;
        for (int j = 0; j < NP; ++j)
            for (uint32_t i = threadIdx.x; i < (1u << L); i += kBlock) fe_store(lo_s + j * (4u << kMlLoBits), i, fe_load(lo + j * lo_stride, i));
        __syncthreads();
        const bool odd = lane & 1;
        const uint32_t own = pair_owned(lane), trips = 1u << (S - 6), lo_mask = (1u << L) - 1;
        const uint64_t n_runs = half >> S;
        const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + wv, nwaves = (uint64_t)gridDim.x * (kBlock / 64);
        const uint4 *in4 = reinterpret_cast<const uint4 *>(src);
        uint4 *out4 = reinterpret_cast<uint4 *>(dst);
        for (uint64_t run = wave; run < n_runs; run += nwaves) {
            Fe acc0[NP], acc1[NP];
            ml_each<NP>([&](auto j) { acc0[j] = fe_zero(), acc1[j] = fe_zero(); });
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
                    pair_scatter(x0, odd, oa, ob);   // plain stores: the next pass or round reads T_r again
                    out4[c0] = oa;
                    out4[c0 + 64] = ob;
                    pair_scatter(x1, odd, oa, ob);
                    out4[c0 + 2 * half] = oa;
                    out4[c0 + 2 * half + 64] = ob;
                } else {
                    x0 = pair_gather(in4[c0], in4[c0 + 64], odd);
                    x1 = pair_gather(in4[c0 + 2 * half], in4[c0 + 2 * half + 64], odd);
                }
                const uint32_t at = ((uint32_t)e0 & lo_mask) + own;
                ml_each<NP>([&](auto j) {
                    const Fe w = fe_load(lo_s + j * (4u << kMlLoBits), at);
                    acc0[j] = fe_add(acc0[j], fe_mul_tt(x0, w, P), P);
                    acc1[j] = fe_add(acc1[j], fe_mul_tt(x1, w, P), P);
                });
            }
            ml_each<NP>([&](auto j) {
                const Fe h = fe_load(hi + j * hi_stride, run >> (L - S));   // wave-uniform address
                tot0[j] = fe_add(tot0[j], fe_mul_tt(acc0[j], h, P), P);
                tot1[j] = fe_add(tot1[j], fe_mul_tt(acc1[j], h, P), P);
            });
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
            ml_each<NP>([&](auto j) {
                const Fe w = fe_load(lo + j * lo_stride, i);
                tot0[j] = fe_mul_tt(x0, w, P);
                tot1[j] = fe_mul_tt(x1, w, P);
            });
        }
    }
    ml_each<NP>([&](auto j) {
        const Fe s0 = fe_wave_sum(tot0[j], P), s1 = fe_wave_sum(tot1[j], P);
        if (lane == 0) {
            wave_sums[(2 * j) * (kBlock / 64) + wv] = s0;
            wave_sums[(2 * j + 1) * (kBlock / 64) + wv] = s1;
        }
    });
    __syncthreads();
    if (threadIdx.x < 2 * NP) {
        Fe s = wave_sums[threadIdx.x * (kBlock / 64)];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) s = fe_add(s, wave_sums[threadIdx.x * (kBlock / 64) + w], P);
        fe_store(partials, 2 * NP * (uint64_t)blockIdx.x + threadIdx.x, s);
    }
}

}  // namespace zk
