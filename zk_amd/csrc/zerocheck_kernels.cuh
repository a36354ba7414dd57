// zerocheck_kernels.cuh -- gfx950 kernels of the zerocheck argument (no reference item; definition: tests/zerocheck_ref.py; host side:
// zerocheck.hip): G(t_0[i], .., t_{k-1}[i]) = 0 on every row, for a gate G that is DATA.
//
// Round j needs, of the k tables T_j (2^(m+1) elements each, variable 0 = the top index bit), the d + 1 sums
//   g_j(X) = sum_{x' < 2^m} W(x') G(T_j(X, x')),   W(x') = eq(x', (tau_{j+1} .. tau_{n-1})),   X = 0 .. d
// with T_j(X, x') = T_j[x'] + X (T_j[2^m + x'] - T_j[x']) per column.  k_zc_round is k_ml_round (mlpcs_kernels.cuh) with the gate in
// the middle: W is read as Hi[x' >> L] Lo[x' & (2^L - 1)] (Lo in LDS, Hi in memory, k_ml_eq_tables makes both for every suffix of tau),
// a wave takes runs of 2^S consecutive x' that share one Hi entry, FOLD reads T_{j-1} as four coalesced streams per column, folds at
// rho_{j-1} and writes T_j once.  Every column is read once per round whatever the gate mentions, and nothing but T_j is written.
//
// The gate is a program (kZcW* words, below) read through scalar loads, so which column a factor names is known at run time only.  An
// array of per-column registers indexed that way goes to scratch; instead every lane parks (value, difference) of its x' for the k
// columns in LDS -- slot 2c and 2c + 1, [slot][half][thread] as 16-byte words, so a wave's access is consecutive -- and the interpreter
// reads operand c from there with a wave-uniform slot number.  A lane touches its own slots only: no barrier.  k * 64 bytes per thread
// next to the 16 KiB Lo table bound the workgroup: 256 threads up to k = 8, 128 up to k = 16 (144 KiB of the CU's 160 at either end).
// The d + 1 accumulators stay in registers: the walk over X is a loop, and the X-th accumulator is picked by d + 1 uniform branches on
// constant indices.
#pragma once
#include "common.cuh"
#include "transcript.cuh"
#include "mlpcs_kernels.cuh"

namespace zk {

constexpr uint32_t kZcMaxCols = 16, kZcMaxTerms = 32, kZcMaxDegree = 6, kZcMaxMentions = 64;
constexpr uint32_t kZcMaxSums = kZcMaxDegree + 1;
// the gate program, 32-bit words in device memory: k, T, d; the terms' lengths; the factors, flat; the terms' kinds; per term nine
// words: the coefficient prepared for fe_mul29 (kind kZcMul), or its eight Montgomery words (kZcConst: the empty term)
constexpr uint32_t kZcWK = 0, kZcWT = 1, kZcWD = 2, kZcWLen = 4, kZcWFactors = kZcWLen + kZcMaxTerms, kZcWKind = kZcWFactors + kZcMaxMentions,
                   kZcWCoeff = kZcWKind + kZcMaxTerms, kZcProgWords = kZcWCoeff + 9 * kZcMaxTerms;
// a term's kind: times the coefficient; coefficient 1 (added as it is); coefficient -1 (subtracted); no factor (the coefficient itself)
enum : uint32_t { kZcMul = 0, kZcPlus = 1, kZcMinus = 2, kZcConst = 3 };
constexpr uint32_t kZcThreadsMax = 256, kZcThreadsWide = 128, kZcWideCols = 8;   // k > kZcWideCols: kZcThreadsWide threads per workgroup
constexpr uint32_t kZcLoBytes = 32u << kMlLoBits;
constexpr uint32_t kZcLdsMax = kZcLoBytes + kZcWideCols * 64 * kZcThreadsMax;

#if defined(__HIPCC__)
typedef const uint32_t __attribute__((address_space(4))) *zc_prog_t;   // constant address space: uniform reads are scalar loads
ZK_D zc_prog_t zc_prog(const uint32_t *p) { return (zc_prog_t)p; }

struct ZcRound {
    const uint32_t *prog;
    const uint64_t *const *cols;   // k pointers in device memory (the caller's tables), or null: column c at src + c * src_stride
    const uint64_t *src;
    uint64_t src_stride;           // in u64 words
    uint64_t *dst;                 // FOLD: column c of T_j at dst + c * dst_stride
    uint64_t dst_stride;
    uint32_t m, S;                 // S (RUN only, 6 <= S <= L): log2 of a run
    const uint64_t *hi, *lo;       // this round's tables: 2^(m-L) and 2^L entries, L = min(m, kMlLoBits)
    const uint64_t *chal;          // FOLD: the challenge record of rho_{j-1}
    uint64_t *partials;            // [gridDim.x][d + 1]
};
ZK_D const uint64_t *zc_col(const ZcRound &a, uint32_t c) {
    if (a.cols) {
        typedef const uint64_t __attribute__((address_space(4))) *ptrs_t;
        return reinterpret_cast<const uint64_t *>(((ptrs_t) reinterpret_cast<const uint64_t *>(a.cols))[c]);
    }
    return a.src + (uint64_t)c * a.src_stride;
}
ZK_D Fe zc_get(const uint4 *stage, uint32_t slot, uint32_t nt, uint32_t tid) {
    const uint4 a = stage[(2 * slot) * nt + tid], b = stage[(2 * slot + 1) * nt + tid];
    Fe r = {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
    return r;
}
ZK_D void zc_put(uint4 *stage, uint32_t slot, uint32_t nt, uint32_t tid, const Fe &e) {
    stage[(2 * slot) * nt + tid] = make_uint4(e.v[0], e.v[1], e.v[2], e.v[3]);
    stage[(2 * slot + 1) * nt + tid] = make_uint4(e.v[4], e.v[5], e.v[6], e.v[7]);
}
// G at the lane's staged values
ZK_D Fe zc_gate(zc_prog_t prog, const uint4 *stage, uint32_t nt, uint32_t tid, const FieldParams &P) {
    const uint32_t T = prog[kZcWT];
    Fe acc = fe_zero();
    uint32_t f = kZcWFactors;
    for (uint32_t i = 0; i < T; ++i) {
        const uint32_t len = prog[kZcWLen + i], kind = prog[kZcWKind + i];
        zc_prog_t cw = prog + kZcWCoeff + 9 * i;
        if (kind == kZcConst) {
            Fe cst;
#pragma unroll
            for (int w = 0; w < 8; ++w) cst.v[w] = cw[w];
            acc = fe_add(acc, cst, P);
            continue;
        }
        Fe prod = zc_get(stage, 2 * prog[f], nt, tid);
        for (uint32_t j = 1; j < len; ++j) prod = fe_mul_tt(prod, zc_get(stage, 2 * prog[f + j], nt, tid), P);
        f += len;
        if (kind == kZcMul) {
            Mul29 c29;
#pragma unroll
            for (int w = 0; w < 9; ++w) c29.l[w] = cw[w];
            prod = fe_mul29(prod, c29, P);
        }
        acc = kind == kZcMinus ? fe_sub(acc, prod, P) : fe_add(acc, prod, P);
    }
    return acc;
}
// the d + 1 sums as named members, one uniform branch each: an array indexed by the walk's X goes to scratch
struct ZcSums {
    Fe s0, s1, s2, s3, s4, s5, s6;
};
#define ZC_EACH(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6)
static_assert(kZcMaxSums == 7, "ZcSums and ZC_EACH name the sums");
ZK_D ZcSums zc_sums_zero() {
    ZcSums z;
#define ZC_ZERO(u) z.s##u = fe_zero();
    ZC_EACH(ZC_ZERO)
#undef ZC_ZERO
    return z;
}
// acc[X] += w G(staged values at X), X = 0 .. d: the values walk by their differences, in place
ZK_D void zc_walk(zc_prog_t prog, uint4 *stage, uint32_t nt, uint32_t tid, uint32_t k, uint32_t d, const Fe &w, ZcSums &acc, const FieldParams &P) {
    for (uint32_t X = 0; X <= d; ++X) {
        const Fe gw = fe_mul_tt(zc_gate(prog, stage, nt, tid, P), w, P);
#define ZC_ADD(u) \
    if (X == u) acc.s##u = fe_add(acc.s##u, gw, P);
        ZC_EACH(ZC_ADD)
#undef ZC_ADD
        if (X < d)
            for (uint32_t c = 0; c < k; ++c) zc_put(stage, 2 * c, nt, tid, fe_add(zc_get(stage, 2 * c, nt, tid), zc_get(stage, 2 * c + 1, nt, tid), P));
    }
}

// FOLD: the launch of round j >= 1 (src: T_{j-1}, 2^(m+2) elements per column); !FOLD: round 0 and zk_mle_gate_sums (src: T_j itself).
// RUN: m >= kMlRunMinBits, blockDim.x = 256 or 128, dynamic LDS = Lo | the stage (k * 64 * blockDim.x bytes); !RUN: one workgroup of 64
// threads, one x' per thread, Lo alone read from memory, dynamic LDS = the stage.
template <bool FOLD, bool RUN>
__global__ __launch_bounds__(kZcThreadsMax) void k_zc_round(ZcRound a, FieldParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zc_smem[];
    __shared__ Fe wave_sums[kZcMaxSums * (kZcThreadsMax / 64)];
    uint64_t *lo_s = reinterpret_cast<uint64_t *>(zc_smem);
    uint4 *stage = reinterpret_cast<uint4 *>(zc_smem + (RUN ? kZcLoBytes : 0));
    const zc_prog_t prog = zc_prog(a.prog);
    const uint32_t k = prog[kZcWK], d = prog[kZcWD];
    const uint32_t m = a.m, nt = blockDim.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wpb = nt >> 6;
    const uint64_t half = 1ull << m;
    Mul29 beta = {};
    if (FOLD) beta = load_challenge29(a.chal);
    ZcSums tot = zc_sums_zero();
    if (RUN) {
        const uint32_t L = m < kMlLoBits ? m : kMlLoBits, S = a.S;
        for (uint32_t i = tid; i < (1u << L); i += nt) fe_store(lo_s, i, fe_load(a.lo, i));
        __syncthreads();
        const bool odd = lane & 1;
        const uint32_t own = pair_owned(lane), trips = 1u << (S - 6), lo_mask = (1u << L) - 1;
        const uint64_t n_runs = half >> S;
        const uint64_t wave = (uint64_t)blockIdx.x * wpb + wv, nwaves = (uint64_t)gridDim.x * wpb;
        for (uint64_t run = wave; run < n_runs; run += nwaves) {
            ZcSums acc = zc_sums_zero();
            for (uint32_t t = 0; t < trips; ++t) {
                const uint64_t e0 = (run << S) + 64 * t;   // the first x' of this trip
                const uint64_t c0 = 2 * e0 + lane;         // element e occupies uint4 slots 2e, 2e + 1
                for (uint32_t c = 0; c < k; ++c) {
                    const uint4 *in4 = reinterpret_cast<const uint4 *>(zc_col(a, c));
                    Fe x0, x1;
                    if (FOLD) {
                        uint4 *out4 = reinterpret_cast<uint4 *>(a.dst + (uint64_t)c * a.dst_stride);
                        Fe v[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint4 p = nt_load16(in4 + c0 + 2 * (uint64_t)j * half), q = nt_load16(in4 + c0 + 2 * (uint64_t)j * half + 64);
                            v[j] = pair_gather(p, q, odd);
                        }
                        x0 = fe_sub(v[0], fe_mul29(fe_sub(v[0], v[2], P), beta, P), P);
                        x1 = fe_sub(v[1], fe_mul29(fe_sub(v[1], v[3], P), beta, P), P);
                        uint4 oa, ob;
                        pair_scatter(x0, odd, oa, ob);   // plain stores: the next round reads T_j again
                        out4[c0] = oa;
                        out4[c0 + 64] = ob;
                        pair_scatter(x1, odd, oa, ob);
                        out4[c0 + 2 * half] = oa;
                        out4[c0 + 2 * half + 64] = ob;
                    } else {
                        x0 = pair_gather(in4[c0], in4[c0 + 64], odd);
                        x1 = pair_gather(in4[c0 + 2 * half], in4[c0 + 2 * half + 64], odd);
                    }
                    zc_put(stage, 2 * c, nt, tid, x0);
                    zc_put(stage, 2 * c + 1, nt, tid, fe_sub(x1, x0, P));
                }
                const Fe w = fe_load(lo_s, ((uint32_t)e0 & lo_mask) + own);
                zc_walk(prog, stage, nt, tid, k, d, w, acc, P);
            }
            const Fe h = fe_load(a.hi, run >> (L - S));   // wave-uniform address
#define ZC_HI(u) \
    if (u <= d) tot.s##u = fe_add(tot.s##u, fe_mul_tt(acc.s##u, h, P), P);
            ZC_EACH(ZC_HI)
#undef ZC_HI
        }
    } else {
        if (tid < half) {   // m < 6: Lo is the whole W
            const uint64_t i = tid;
            for (uint32_t c = 0; c < k; ++c) {
                const uint64_t *src = zc_col(a, c);
                Fe x0, x1;
                if (FOLD) {
                    uint64_t *dst = a.dst + (uint64_t)c * a.dst_stride;
                    const Fe a0 = fe_load(src, i), a1 = fe_load(src, i + half), a2 = fe_load(src, i + 2 * half), a3 = fe_load(src, i + 3 * half);
                    x0 = fe_sub(a0, fe_mul29(fe_sub(a0, a2, P), beta, P), P);
                    x1 = fe_sub(a1, fe_mul29(fe_sub(a1, a3, P), beta, P), P);
                    fe_store(dst, i, x0);
                    fe_store(dst, i + half, x1);
                } else {
                    x0 = fe_load(src, i);
                    x1 = fe_load(src, i + half);
                }
                zc_put(stage, 2 * c, nt, tid, x0);
                zc_put(stage, 2 * c + 1, nt, tid, fe_sub(x1, x0, P));
            }
            zc_walk(prog, stage, nt, tid, k, d, fe_load(a.lo, i), tot, P);
        }
    }
#define ZC_WAVE(u)                                                  \
    if (u <= d) {                                                   \
        const Fe s = fe_wave_sum(tot.s##u, P);                      \
        if (lane == 0) wave_sums[u * (kZcThreadsMax / 64) + wv] = s; \
    }
    ZC_EACH(ZC_WAVE)
#undef ZC_WAVE
    __syncthreads();
    if (tid <= d) {
        Fe s = wave_sums[tid * (kZcThreadsMax / 64)];
        for (uint32_t w = 1; w < wpb; ++w) s = fe_add(s, wave_sums[tid * (kZcThreadsMax / 64) + w], P);
        fe_store(a.partials, (uint64_t)blockIdx.x * (d + 1) + tid, s);
    }
}

// ---- the proof's transcript on the device ------------------------------------------------------------------------------------------------
// tau_0 .. tau_{n-1} by sample_field_element, one wave
static __global__ __launch_bounds__(64) void k_zc_tau(WordSponge *__restrict__ gsp, uint32_t n, uint64_t *__restrict__ tau, FieldParams P) {
    const LaneKeccak L = lane_keccak_init();
    LaneSponge sp = lane_sponge_load(gsp, L);
    for (uint32_t j = 0; j < n; ++j) {
        const Fe t = challenge_fe_of(lane_squeeze_x(sp, L), P);
        if (L.lane == 0) fe_store(tau, j, t);
    }
    lane_sponge_store(gsp, sp, L);
}
// The end of round j: the [nblocks][ns] partials -> g_j (out_rp: its place in the proof block), four waves sharing the sums; then wave 0
// absorbs g_j and squeezes rho_j: Montgomery form to out_ch (the point's slot in the block) and the record at d_challenge, prepared
// for fe_mul29, where the next round kernel and the finish read it.
static __global__ __launch_bounds__(kBlock) void k_zc_step(const uint64_t *__restrict__ partials, uint32_t nblocks, uint32_t ns, WordSponge *__restrict__ gsp,
                                                            uint64_t *__restrict__ out_rp, uint64_t *__restrict__ out_ch, uint64_t *__restrict__ d_challenge,
                                                            FieldParams P) {
    __shared__ Fe fin[kZcMaxSums + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool wave0 = __builtin_amdgcn_readfirstlane(wave) == 0;
    const LaneKeccak L = lane_keccak_init();
    LaneSponge sp = {0, 0};
    if (wave0) sp = lane_sponge_load(gsp, L);   // in flight while the partials are added up
    for (uint32_t t = wave; t < ns; t += kBlock / 64) {
        Fe s = fe_zero();
        for (uint32_t b = lane; b < nblocks; b += 64) s = fe_add(s, fe_load(partials, (uint64_t)b * ns + t), P);
        s = fe_wave_sum(s, P);
        if (lane == 0) fin[t] = s;
    }
    __syncthreads();
    if (threadIdx.x >= kBlock - 64 && (uint32_t)lane < ns) fe_store(out_rp, lane, fin[lane]);
    if (wave0) {
        lane_absorb_elems(sp, L, fin, ns, P);
        Mul29 ch29;
        Fe ch;
        challenge_forms(lane_squeeze_x(sp, L), (uint32_t)lane, P, ch29, ch);   // lane 0: multiplier form, lane 16: Montgomery form
        publish_challenge_forms(d_challenge, out_ch, ch, ch29, (uint32_t)lane);
        lane_sponge_store(gsp, sp, L);
    }
}
// v_c = T_{n-1}[c](rho_{n-1}), c < k: the proof's last k elements, which are the claims.  (The definition absorbs them; nothing is drawn
// from the transcript afterwards, so the device leaves that out.)
static __global__ __launch_bounds__(64) void k_zc_finish(const uint64_t *const *__restrict__ cols, const uint64_t *__restrict__ src, uint64_t src_stride, uint32_t k,
                                                          const uint64_t *__restrict__ chal, uint64_t *__restrict__ out, FieldParams P) {
    const uint32_t c = threadIdx.x;
    if (c >= k) return;
    const Mul29 rho = load_challenge29(chal);
    const uint64_t *t = cols ? cols[c] : src + (uint64_t)c * src_stride;
    const Fe a = fe_load(t, 0), b = fe_load(t, 1);
    fe_store(out, c, fe_sub(a, fe_mul29(fe_sub(a, b, P), rho, P), P));
}
#endif

}  // namespace zk
