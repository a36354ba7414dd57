// sumcheck_kernels.cuh -- the sumcheck prover's own kernels (host schedule: sumcheck.hip): the fold at a device-resident challenge, the
// second stage of a round with its transcript step, the classic finishers, the sponge store, the sharded prover's lane transcript and
// gather, the factor values at the point, and the publication of a proof block to pinned host memory.  The round kernels proper are
// round_kernels.cuh (rounds.hip) and pipe_kernels.cuh (pipe.hip); the MLE fold / evaluate family is kernels.cuh (capi.hip).
#pragma once
#include "common.cuh"
#include "keccak.hpp"
#include "transcript.cuh"

namespace zk {

// same fold with the challenge read from device memory (produced by the on-device transcript); m = variables of `in`,
// always the MSB fold.  `pairs` = 2^(m-1).
__global__ __launch_bounds__(kBlock) void k_fold_dev(const uint64_t *in, uint64_t *out, uint64_t pairs, uint32_t m,
                                                     FieldParams P, const uint64_t *__restrict__ rptr) {
    (void)m;
    const Mul29 r = load_challenge29(rptr);
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < pairs; j += stride) {
        const Fe lo = fe_load(in, j);
        const Fe hi = fe_load(in, j + pairs);
        fe_store(out, j, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));
    }
}

// Second stage of a round: one workgroup adds the per-block partials -> ns sums (Montgomery form); then, on lane 0,
//   out_rp   != null : store the sums (the round polynomial);
//   lanes    != null : store them as 8 zero-extended 32-bit digits per element (uint64 lanes) for the cross-GPU
//                      all-reduce (RCCL has no mod-p sum; integer lane sums cannot overflow);
//   sponge   != null : run the transcript step and publish the challenge.
// init (optional, a kernel ARGUMENT): the proof's initial sponge state.  The tail that closes round 0 then takes the state from its own
// arguments instead of from *sponge, and clears the two counters at zero2 -- the launch that used to do both in front of round 0
// (k_store_sponge) disappears from the single proof's serial chain.  25 selects on SGPR operands: a dynamic index into a by-value
// argument would send it through scratch.
ZK_D LaneSponge lane_sponge_from_arg(const WordSponge &w, const LaneKeccak &L) {
    LaneSponge sp;
    sp.a = 0;
#pragma unroll
    for (int i = 0; i < 25; ++i)
        if (L.index == i) sp.a = w.s[i];
    sp.pos = w.pos;
    return sp;
}
ZK_D void round_tail_body(const uint64_t *__restrict__ partials, uint32_t nblocks, uint32_t ns, WordSponge *__restrict__ sponge,
                          uint64_t *__restrict__ out_rp, uint64_t *__restrict__ out_ch, uint64_t *__restrict__ d_challenge,
                          uint64_t *__restrict__ lanes, const FieldParams &P, const TailDerive &dv, const WordSponge *init = nullptr,
                          uint64_t *__restrict__ zero2 = nullptr) {
    __shared__ Fe fin[256];
    __shared__ Fe claim;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool wave0 = __builtin_amdgcn_readfirstlane(wave) == 0;
    const bool derive1 = dv.prev_rp != nullptr;   // the partials carry no t = 1 sums (k_round_kd SKIP1)
    // wave 0 fetches the sponge first, so that load is in flight while the partials are reduced
    const LaneKeccak L = lane_keccak_init();
    LaneSponge sp = {0, 0};
    if (sponge && wave0) sp = init ? lane_sponge_from_arg(*init, L) : lane_sponge_load(sponge, L);
    if (init && zero2 && threadIdx.x >= 64 && threadIdx.x < 66) zero2[threadIdx.x - 64] = 0;
    // wave w owns the sums t = w, w+4, ...: lanes stride over the blocks' partials, one VALU wave reduction, one barrier
    for (uint32_t t = wave; t < ns; t += kBlock / 64) {
        if (derive1 && t == 1 && (dv.claim || dv.local_only)) {
            // this wave would own t = 1: the round kernel's claim workgroup has evaluated S_prev(r_prev) already -- or nobody needs
            // it here: a sharded round derives S(1) after the all-reduce (k_lanes_transcript reads or evaluates the claim itself)
            if (lane == 0) {
                if (dv.local_only) fin[1] = fe_zero();
                else claim = fe_load(dv.claim, 0);
            }
            continue;
        }
        if (derive1 && t == 1) {
            // this wave would own t = 1: it evaluates the previous round polynomial at the previous challenge instead,
            //   claim = sum_t prev[t] * w[t] * prod_{u != t} (r - u)   (lane t takes term t; D + 1 multiplies deep)
            const Fe r = fe_load(dv.prev_chal, 0);
            Fe term = fe_zero();
            if ((uint32_t)lane < ns) {
                Fe one;
#pragma unroll
                for (int i = 0; i < 8; ++i) one.v[i] = P.r1[i];
                const Fe wt = fe_load(dv.w, lane);
                term = fe_mul(fe_load(dv.prev_rp, lane), wt, P);
                Fe node = fe_zero();   // Montgomery form of u
                for (uint32_t u = 0; u < ns; ++u) {
                    if (u != (uint32_t)lane) term = fe_mul(term, fe_sub(r, node, P), P);
                    node = fe_add(node, one, P);
                }
            }
            term = fe_wave_sum(term, P, 8);
            if (lane == 0) claim = term;
            continue;
        }
        Fe s = fe_zero();
        for (uint32_t b = lane; b < nblocks; b += 8 * 64) {   // eight independent loads in flight, then a tree of adds
            Fe x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = b + u * 64 < nblocks ? fe_load(partials, (uint64_t)(b + u * 64) * ns + t) : fe_zero();
            const Fe lo = fe_add(fe_add(x[0], x[1], P), fe_add(x[2], x[3], P), P), hi = fe_add(fe_add(x[4], x[5], P), fe_add(x[6], x[7], P), P);
            s = fe_add(s, fe_add(lo, hi, P), P);
        }
        s = fe_wave_sum(s, P);
        if (lane == 0) fin[t] = s;
    }
    __syncthreads();
    if ((derive1 || dv.lead) && !dv.local_only) {
        if (threadIdx.x == 0) {
            if (derive1) fin[1] = fe_sub(claim, fin[0], P);        // S(1) = S_prev(r_prev) - S(0)
            if (dv.lead) fin[dv.lead] = lead_rebuild(dv.lead, fin, P);   // slot D held the leading coefficient (k_round_kd LEAD)
        }
        __syncthreads();
    }
    if (threadIdx.x == kBlock - 64) {   // the last wave stores the round polynomial while wave 0 runs the transcript
        for (uint32_t t = 0; t < ns; ++t) {
            if (out_rp) fe_store(out_rp, t, fin[t]);
            if (lanes)
                for (int i = 0; i < 8; ++i) lanes[8 * t + i] = (uint64_t)fin[t].v[i];
        }
    }
    if (sponge && wave0) {
        lane_absorb_elems(sp, L, fin, ns, P);
        Mul29 ch29;
        Fe ch;
        challenge_forms(lane_squeeze_x(sp, L), (uint32_t)lane, P, ch29, ch);   // lane 0: multiplier form, lane 16: Montgomery form
        publish_challenge_forms(d_challenge, out_ch, ch, ch29, (uint32_t)lane);
        lane_sponge_store(sponge, sp, L);
    }
}
__global__ __launch_bounds__(kBlock) void k_round_tail(const uint64_t *__restrict__ partials, uint32_t nblocks, uint32_t ns,
                                                       WordSponge *__restrict__ sponge, uint64_t *__restrict__ out_rp,
                                                       uint64_t *__restrict__ out_ch, uint64_t *__restrict__ d_challenge,
                                                       uint64_t *__restrict__ lanes, FieldParams P, TailDerive dv = {}) {
    round_tail_body(partials, nblocks, ns, sponge, out_rp, out_ch, d_challenge, lanes, P, dv);
}
// the tail of round 0 of a single proof: the initial sponge state arrives as an argument (round_tail_body)
__global__ __launch_bounds__(kBlock) void k_round_tail_init(const uint64_t *__restrict__ partials, uint32_t nblocks, uint32_t ns,
                                                            WordSponge *__restrict__ sponge, uint64_t *__restrict__ out_rp,
                                                            uint64_t *__restrict__ out_ch, uint64_t *__restrict__ d_challenge, FieldParams P,
                                                            TailDerive dv, WordSponge init, uint64_t *__restrict__ zero2) {
    round_tail_body(partials, nblocks, ns, sponge, out_rp, out_ch, d_challenge, nullptr, P, dv, &init, zero2);
}
// batched form (zk_sumcheck_prove_batch): grid (1, proofs), the B transcript steps of a round side by side
struct TailSlot {
    const uint64_t *partials;
    WordSponge *sponge;
    uint64_t *out_rp, *out_ch, *d_challenge;
    TailDerive dv;
};
__global__ __launch_bounds__(kBlock) void k_round_tail_b(BatchOf<TailSlot> b, uint32_t nblocks, uint32_t ns, FieldParams P) {
    const TailSlot &a = b.a[blockIdx.y];
    round_tail_body(a.partials, nblocks, ns, a.sponge, a.out_rp, a.out_ch, a.d_challenge, nullptr, P, a.dv);
}

// ---- finisher: all remaining rounds of the prover in ONE launch, once the tables are small ---------------------------
// A round on a tiny table is pure latency (two launches, a trip through HBM for 96 bytes of sums, the serial transcript).
// One workgroup keeps the K tables (<= 2^kFinishVars elements each) in LDS and the sponge in the registers of wave 0 and
// loops: sums -> workgroup reduction -> transcript step -> fold in LDS (prover.rs:44-68, unchanged semantics).
//   pending != 0: the tables in HBM still need the previous challenge applied (prover.rs:64) while they are loaded.
//   out_final: optional, K elements: the factors evaluated at the full challenge point.
constexpr int kFinishVars = 9;
template <int K, int D>
__global__ __launch_bounds__(kBlock) void k_finish(FactorPtrs fp, uint32_t m_in, int pending, FieldParams P,
                                                   uint64_t *d_challenge, WordSponge *gsponge, uint64_t *out_rp, uint64_t *out_ch,
                                                   uint64_t *out_final) {
    constexpr int NS = D + 1;
    // all LDS is carved from the dynamic region at 16-byte aligned offsets (no static __shared__ in front of it)
    extern __shared__ __attribute__((aligned(16))) unsigned char fin_smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool wave0 = __builtin_amdgcn_readfirstlane(wave) == 0;
    uint32_t m = pending ? m_in - 1 : m_in;       // variables of the tables held in LDS
    const uint32_t n_elems = 1u << m;
    uint64_t *tab = reinterpret_cast<uint64_t *>(fin_smem);                 // K tables of 2^m elements, 4 u64 each
    unsigned char *carve = fin_smem + (size_t)K * n_elems * 32;
    uint32_t(*red)[NS][8] = reinterpret_cast<uint32_t(*)[NS][8]>(carve);    // [waves][NS][8]
    Fe *fin = reinterpret_cast<Fe *>(carve + (kBlock / 64) * NS * 32);
    Mul29 *sh_r29p = reinterpret_cast<Mul29 *>(carve + (kBlock / 64) * NS * 32 + NS * 32);
    // ---- load (and fold when pending) ----
    if (pending) {
        const Mul29 r = load_challenge29(d_challenge);
#pragma unroll
        for (int f = 0; f < K; ++f)
            for (uint32_t j = tid; j < n_elems; j += kBlock) {
                const Fe lo = fe_load(fp.in[f], j), hi = fe_load(fp.in[f], j + n_elems);
                fe_store(tab + (size_t)f * n_elems * 4, j, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));
            }
    } else {
#pragma unroll
        for (int f = 0; f < K; ++f)
            for (uint32_t j = tid; j < n_elems; j += kBlock) fe_store(tab + (size_t)f * n_elems * 4, j, fe_load(fp.in[f], j));
    }
    LaneKeccak L = lane_keccak_init();
    LaneSponge sp = {0, 0};
    if (wave0) sp = lane_sponge_load(gsponge, L);
    __syncthreads();
    uint32_t round = 0;
    while (m >= 1) {
        const uint32_t q = 1u << (m - 1);
        if (q <= 128) {
            // ---- one evaluation point per WAVE: wave t forms S_t over all pairs (k - 1 multiplies per pair instead of
            // (D + 1)(k - 1) on one lane), reduces it on the VALU and owns fin[t]: no cross-wave exchange ----
            for (uint32_t t = wave; t < (uint32_t)NS; t += kBlock / 64) {
                Fe s = fe_zero();
                for (uint32_t j = lane; j < q; j += 64) {
                    Fe prod;
#pragma unroll
                    for (int f = 0; f < K; ++f) {
                        const uint64_t *T = tab + (size_t)f * n_elems * 4;
                        const Fe lo = fe_load(T, j), hi = fe_load(T, j + q);
                        Fe v = lo;
                        if (t >= 1) v = hi;
                        if (t >= 2) {
                            const Fe diff = fe_sub(hi, lo, P);
                            for (uint32_t u = 1; u < t; ++u) v = fe_add(v, diff, P);
                        }
                        prod = (f == 0) ? v : fe_mul(prod, v, P);
                    }
                    s = fe_add(s, prod, P);
                }
                s = fe_wave_sum(s, P, q < 64 ? q : 64);
                if (lane == 0) {
                    fin[t] = s;
                    fe_store(out_rp, (uint64_t)round * NS + t, s);
                }
            }
            __syncthreads();
        } else {
        // ---- sums over the pairs (j, j+q) ----
        Fe sum[NS];
#pragma unroll
        for (int t = 0; t < NS; ++t) sum[t] = fe_zero();
        for (uint32_t j = tid; j < q; j += kBlock) {
            Fe prod[NS];
#pragma unroll
            for (int f = 0; f < K; ++f) {
                const uint64_t *T = tab + (size_t)f * n_elems * 4;
                const Fe lo = fe_load(T, j), hi = fe_load(T, j + q);
                const Fe diff = fe_sub(hi, lo, P);
                Fe v = lo;
#pragma unroll
                for (int t = 0; t < NS; ++t) {
                    if (t == 1) v = hi;
                    else if (t > 1) v = fe_add(v, diff, P);
                    prod[t] = (f == 0) ? v : fe_mul(prod[t], v, P);
                }
            }
#pragma unroll
            for (int t = 0; t < NS; ++t) sum[t] = fe_add(sum[t], prod[t], P);
        }
        // ---- workgroup reduction -> fin[] ----
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            sum[t] = fe_wave_sum(sum[t], P, q < 64 ? q : 64);   // lanes >= q hold zero: empty levels are skipped
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) red[wave][t][i] = sum[t].v[i];
            }
        }
        __syncthreads();
        if (tid < NS) {
            Fe acc;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc.v[i] = red[0][tid][i];
            if (q > 64) {
                for (int w = 1; w < kBlock / 64; ++w) {
                    Fe o;
#pragma unroll
                    for (int i = 0; i < 8; ++i) o.v[i] = red[w][tid][i];
                    acc = fe_add(acc, o, P);
                }
            }
            fin[tid] = acc;
            fe_store(out_rp, (uint64_t)round * NS + tid, acc);
        }
        __syncthreads();
        }
        // ---- transcript step on wave 0, challenge to everyone through LDS ----
        if (wave0) {
            lane_absorb_elems(sp, L, fin, NS, P);
            Mul29 ch29;
            Fe ch;
            challenge_forms(lane_squeeze_x(sp, L), lane, P, ch29, ch);   // lane 0: multiplier form, lane 16: Montgomery form
            if (lane == 16) fe_store(out_ch, round, ch);
            if (lane == 0) *sh_r29p = ch29;
            if (m == 1) publish_challenge_forms(d_challenge, nullptr, ch, ch29, lane);   // last one: for the sharded tail
        }
        __syncthreads();
        // ---- fold at the challenge, in LDS (prover.rs:64); the fold after the last round is dropped by the reference
        if (m > 1) {
            Mul29 r;
#pragma unroll
            for (int i = 0; i < 9; ++i) r.l[i] = __builtin_amdgcn_readfirstlane(sh_r29p->l[i]);
            // work items (factor, index): every lane has at most ceil(k*q / 256) multiplies
            const uint32_t lq = m - 1;
            for (uint32_t i = tid; i < ((uint32_t)K << lq); i += kBlock) {
                uint64_t *T = tab + (size_t)(i >> lq) * n_elems * 4;
                const uint32_t j = i & (q - 1);
                const Fe lo = fe_load(T, j), hi = fe_load(T, j + q);
                fe_store(T, j, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));
            }
            __syncthreads();
        }
        --m;
        ++round;
    }
    if (wave0) lane_sponge_store(gsponge, sp, L);
    // out_final != null: the factors at the challenge point, i.e. the fold after the last round (the reference computes
    // and drops it, prover.rs:64; a layered driver needs W(u))
    if (out_final && tid < K) {
        Mul29 r;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.l[i] = sh_r29p->l[i];
        const uint64_t *T = tab + (size_t)tid * n_elems * 4;
        const Fe lo = fe_load(T, 0), hi = fe_load(T, 1);
        fe_store(out_final, tid, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));
    }
}

// The same finisher for a SUM of products (zk_sumcheck_prove_terms; a GKR layer polynomial): the factor list is grouped into
// terms at run time, each pair contributes sum_i prod_{f in term i}.
template <int D>
__global__ __launch_bounds__(kBlock) void k_finish_terms(FactorPtrs fp, TermSpec ts, uint32_t m_in, int pending, FieldParams P,
                                                   uint64_t *d_challenge, WordSponge *gsponge, uint64_t *out_rp, uint64_t *out_ch,
                                                   uint64_t *out_final) {
    constexpr int NS = D + 1;
    int K = 0;   // factors in all (runtime here)
    for (int i = 0; i < ts.n_terms; ++i) K += ts.term_k[i];
    // all LDS is carved from the dynamic region at 16-byte aligned offsets (no static __shared__ in front of it)
    extern __shared__ __attribute__((aligned(16))) unsigned char fin_smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool wave0 = __builtin_amdgcn_readfirstlane(wave) == 0;
    uint32_t m = pending ? m_in - 1 : m_in;       // variables of the tables held in LDS
    const uint32_t n_elems = 1u << m;
    uint64_t *tab = reinterpret_cast<uint64_t *>(fin_smem);                 // K tables of 2^m elements, 4 u64 each
    unsigned char *carve = fin_smem + (size_t)K * n_elems * 32;
    uint32_t(*red)[NS][8] = reinterpret_cast<uint32_t(*)[NS][8]>(carve);    // [waves][NS][8]
    Fe *fin = reinterpret_cast<Fe *>(carve + (kBlock / 64) * NS * 32);
    Mul29 *sh_r29p = reinterpret_cast<Mul29 *>(carve + (kBlock / 64) * NS * 32 + NS * 32);
    // ---- load (and fold when pending) ----
    if (pending) {
        const Mul29 r = load_challenge29(d_challenge);
#pragma unroll
        for (int f = 0; f < K; ++f)
            for (uint32_t j = tid; j < n_elems; j += kBlock) {
                const Fe lo = fe_load(fp.in[f], j), hi = fe_load(fp.in[f], j + n_elems);
                fe_store(tab + (size_t)f * n_elems * 4, j, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));
            }
    } else {
#pragma unroll
        for (int f = 0; f < K; ++f)
            for (uint32_t j = tid; j < n_elems; j += kBlock) fe_store(tab + (size_t)f * n_elems * 4, j, fe_load(fp.in[f], j));
    }
    LaneKeccak L = lane_keccak_init();
    LaneSponge sp = {0, 0};
    if (wave0) sp = lane_sponge_load(gsponge, L);
    __syncthreads();
    uint32_t round = 0;
    while (m >= 1) {
        const uint32_t q = 1u << (m - 1);
        if (q <= 128) {
            // ---- one evaluation point per WAVE (see k_finish) ----
            for (uint32_t t = wave; t < (uint32_t)NS; t += kBlock / 64) {
                Fe s = fe_zero();
                for (uint32_t j = lane; j < q; j += 64) {
                    int f = 0;
                    for (int i = 0; i < ts.n_terms; ++i) {
                        Fe prod;
                        for (int g = 0; g < ts.term_k[i]; ++g, ++f) {
                            const uint64_t *T = tab + (size_t)f * n_elems * 4;
                            const Fe lo = fe_load(T, j), hi = fe_load(T, j + q);
                            Fe v = lo;
                            if (t >= 1) v = hi;
                            if (t >= 2) {
                                const Fe diff = fe_sub(hi, lo, P);
                                for (uint32_t u = 1; u < t; ++u) v = fe_add(v, diff, P);
                            }
                            prod = (g == 0) ? v : fe_mul(prod, v, P);
                        }
                        s = fe_add(s, prod, P);
                    }
                }
                s = fe_wave_sum(s, P, q < 64 ? q : 64);
                if (lane == 0) {
                    fin[t] = s;
                    fe_store(out_rp, (uint64_t)round * NS + t, s);
                }
            }
            __syncthreads();
        } else {
        // ---- sums over the pairs (j, j+q) ----
        Fe sum[NS];
#pragma unroll
        for (int t = 0; t < NS; ++t) sum[t] = fe_zero();
        for (uint32_t j = tid; j < q; j += kBlock) {
            int f = 0;
            for (int i = 0; i < ts.n_terms; ++i) {
                Fe prod[NS];
                for (int g = 0; g < ts.term_k[i]; ++g, ++f) {
                    const uint64_t *T = tab + (size_t)f * n_elems * 4;
                    const Fe lo = fe_load(T, j), hi = fe_load(T, j + q);
                    const Fe diff = fe_sub(hi, lo, P);
                    Fe v = lo;
#pragma unroll
                    for (int t = 0; t < NS; ++t) {
                        if (t == 1) v = hi;
                        else if (t > 1) v = fe_add(v, diff, P);
                        prod[t] = (g == 0) ? v : fe_mul(prod[t], v, P);
                    }
                }
#pragma unroll
                for (int t = 0; t < NS; ++t) sum[t] = fe_add(sum[t], prod[t], P);
            }
        }
        // ---- workgroup reduction -> fin[] ----
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            sum[t] = fe_wave_sum(sum[t], P, q < 64 ? q : 64);   // lanes >= q hold zero: empty levels are skipped
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) red[wave][t][i] = sum[t].v[i];
            }
        }
        __syncthreads();
        if (tid < NS) {
            Fe acc;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc.v[i] = red[0][tid][i];
            if (q > 64) {
                for (int w = 1; w < kBlock / 64; ++w) {
                    Fe o;
#pragma unroll
                    for (int i = 0; i < 8; ++i) o.v[i] = red[w][tid][i];
                    acc = fe_add(acc, o, P);
                }
            }
            fin[tid] = acc;
            fe_store(out_rp, (uint64_t)round * NS + tid, acc);
        }
        __syncthreads();
        }
        // ---- transcript step on wave 0, challenge to everyone through LDS ----
        if (wave0) {
            lane_absorb_elems(sp, L, fin, NS, P);
            Mul29 ch29;
            Fe ch;
            challenge_forms(lane_squeeze_x(sp, L), lane, P, ch29, ch);   // lane 0: multiplier form, lane 16: Montgomery form
            if (lane == 16) fe_store(out_ch, round, ch);
            if (lane == 0) *sh_r29p = ch29;
            if (m == 1) publish_challenge_forms(d_challenge, nullptr, ch, ch29, lane);   // last one: for the sharded tail
        }
        __syncthreads();
        // ---- fold at the challenge, in LDS (prover.rs:64); the fold after the last round is dropped by the reference
        if (m > 1) {
            Mul29 r;
#pragma unroll
            for (int i = 0; i < 9; ++i) r.l[i] = __builtin_amdgcn_readfirstlane(sh_r29p->l[i]);
            const uint32_t lq = m - 1;
            for (uint32_t i = tid; i < ((uint32_t)K << lq); i += kBlock) {
                uint64_t *T = tab + (size_t)(i >> lq) * n_elems * 4;
                const uint32_t j = i & (q - 1);
                const Fe lo = fe_load(T, j), hi = fe_load(T, j + q);
                fe_store(T, j, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));
            }
            __syncthreads();
        }
        --m;
        ++round;
    }
    if (wave0) lane_sponge_store(gsponge, sp, L);
    // out_final != null: the factors at the challenge point, i.e. the fold after the last round (the reference computes
    // and drops it, prover.rs:64; a layered driver needs W(u))
    if (out_final && (int)tid < K) {
        Mul29 r;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.l[i] = sh_r29p->l[i];
        const uint64_t *T = tab + (size_t)tid * n_elems * 4;
        const Fe lo = fe_load(T, 0), hi = fe_load(T, 1);
        fe_store(out_final, tid, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));
    }
}

// the prover's initial sponge state, passed by value in the kernel arguments
// zero2 (optional): two uint64 words cleared by the same launch (the pipelined rounds' last-block-done counters: a 16-byte
// hipMemsetAsync is a launch of its own on the stream)
ZK_D void store_sponge_body(const WordSponge &w, WordSponge *__restrict__ dst, uint64_t *__restrict__ zero2) {
    if (threadIdx.x < 25) dst->s[threadIdx.x] = w.s[threadIdx.x];
    if (threadIdx.x == 0) {
        dst->pos = w.pos;
        dst->pad_ = 0;
    }
    if (zero2 && threadIdx.x >= 32 && threadIdx.x < 34) zero2[threadIdx.x - 32] = 0;
}
__global__ void k_store_sponge(WordSponge w, WordSponge *__restrict__ dst, uint64_t *__restrict__ zero2) { store_sponge_body(w, dst, zero2); }
struct SpongeSlot {
    WordSponge w;
    WordSponge *dst;
    uint64_t *zero2;
};
__global__ void k_store_sponge_b(BatchOf<SpongeSlot> b) {
    const SpongeSlot &a = b.a[blockIdx.y];
    store_sponge_body(a.w, a.dst, a.zero2);
}

// Sharded prover, after the all-reduce: lanes hold sums over ranks of 32-bit digits.  Carry-propagate, reduce mod p
// (value < world * p, world <= 2^16), then the same transcript step.  One wave.
// dv: the round kernels left out the t = 1 sums (prev_rp != null: S(1) = S_prev(r_prev) - S(0), the identity holds for the GLOBAL
// sums) and / or put the leading coefficient in slot D (lead: the slot is linear in the shards, so its all-reduced value is the
// global leading coefficient) -- the same derivations k_round_tail makes on one GPU, made here on the all-reduced values.
__global__ __launch_bounds__(128) void k_lanes_transcript(const uint64_t *__restrict__ lanes, uint32_t ns, WordSponge *__restrict__ sponge,
                                                          uint64_t *__restrict__ out_rp, uint64_t *__restrict__ out_ch,
                                                          uint64_t *__restrict__ d_challenge, FieldParams P, TailDerive dv) {
    __shared__ Fe fin[256];
    __shared__ Fe claim_s;
    if (blockIdx.x != 0 || threadIdx.x >= 128) return;   // two waves, wave-uniform control flow
    const uint32_t lane = threadIdx.x & 63;
    const bool wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
    const bool fixup = dv.prev_rp != nullptr || dv.lead != 0;
    // wave 0 fetches the sponge first, so that load is in flight while the lanes are reduced (as k_round_tail does)
    const LaneKeccak L = lane_keccak_init();
    LaneSponge sp = {0, 0};
    if (wave0) {
        sp = lane_sponge_load(sponge, L);
        Fe claim_early = fe_zero();
        if (dv.prev_rp && dv.claim) claim_early = fe_load(dv.claim, 0);   // evaluated by k_round_tail in front of the all-reduce; in flight with the lanes
        // lane t takes sum t (t, t + 64, ...): the carry propagation and the 17-step ladder run once for all sums of a batch instead
        // of once per sum on every lane (the ladder is ~350 dependent steps: ~1 us of the serial chain of every exchanging round)
        for (uint32_t t0 = 0; t0 < ns; t0 += 64) {
            const uint32_t t = t0 + lane < ns ? t0 + lane : ns - 1;
            uint32_t v[9];
            uint64_t carry = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                carry += lanes[8 * t + i];
                v[i] = (uint32_t)carry;
                carry >>= 32;
            }
            v[8] = (uint32_t)carry;
            if (dv.log_world <= 3) ladder9<4>(v, P);   // value < 2^log_world * p: up to eight ranks 16p .. p suffices (wave-uniform branch)
            else ladder9<16>(v, P);
            Fe r;
#pragma unroll
            for (int i = 0; i < 8; ++i) r.v[i] = v[i];
            if (t0 + lane < ns) {
                fin[t] = r;
                if (!fixup) fe_store(out_rp, t, r);
            }
        }
        if (dv.prev_rp && dv.claim && lane == 0) claim_s = claim_early;
    } else if (dv.prev_rp && !dv.claim) {
        // wave 1, beside the ladder (nothing here depends on the lanes): claim = S_prev(r_prev) = sum_t prev[t] * w[t] * prod_{u != t} (r_prev - u),
        // lane t takes term t (fast degrees only: ns <= 5)
        const Fe r = fe_load(dv.prev_chal, 0);
        Fe term = fe_zero();
        if (lane < ns) {
            Fe one;
#pragma unroll
            for (int i = 0; i < 8; ++i) one.v[i] = P.r1[i];
            term = fe_mul(fe_load(dv.prev_rp, lane), fe_load(dv.w, lane), P);
            Fe node = fe_zero();   // Montgomery form of u
            for (uint32_t u = 0; u < ns; ++u) {
                if (u != lane) term = fe_mul(term, fe_sub(r, node, P), P);
                node = fe_add(node, one, P);
            }
        }
        const Fe claim = fe_wave_sum(term, P, 8);   // valid in lane 0
        if (lane == 0) claim_s = claim;
    }
    __syncthreads();
    if (!wave0) return;
    if (fixup) {
        if (lane == 0) {
            if (dv.prev_rp) fin[1] = fe_sub(claim_s, fin[0], P);             // S(1) = S_prev(r_prev) - S(0), on the GLOBAL sums
            if (dv.lead) fin[dv.lead] = lead_rebuild(dv.lead, fin, P);        // slot D held the (global) leading coefficient
        }
        __builtin_amdgcn_wave_barrier();   // same wave: LDS operations execute in order
        if (lane < ns) fe_store(out_rp, lane, fin[lane]);
    }
    lane_absorb_elems(sp, L, fin, ns, P);
    Mul29 ch29;
    Fe ch;
    challenge_forms(lane_squeeze_x(sp, L), (uint32_t)L.lane, P, ch29, ch);
    publish_challenge_forms(d_challenge, out_ch, ch, ch29, (uint32_t)L.lane);
    lane_sponge_store(sponge, sp, L);
}

// interleave the all-gathered shard tables [rank][factor][2^s] into k tables of world * 2^s elements:
// table_f[local * world + rank] = gathered[rank][f][local]  (global index = local * world + rank)
__global__ __launch_bounds__(kBlock) void k_gather_to_tables(const uint64_t *__restrict__ gathered, FactorPtrs fp, uint32_t k,
                                                             uint32_t world, uint32_t s) {
    const uint64_t per_rank = (uint64_t)k << s, total = per_rank * world, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const uint64_t rank = i / per_rank, rem = i % per_rank;
        const uint32_t f = (uint32_t)(rem >> s);
        const uint64_t local = rem & ((1ull << s) - 1);
        fe_store(fp.out[f], local * world + rank, fe_load(gathered, i));
    }
}

// The factors of a sum-of-products sumcheck at the challenge point: the fold after the LAST round (prover.rs:64), which
// the reference computes and drops; a layered driver needs it (W(u), W(v)).  tables hold 2 elements each.
__global__ void k_final_evals(FactorPtrs fp, uint32_t k, const uint64_t *__restrict__ d_challenge, uint64_t *__restrict__ out,
                              FieldParams P) {
    const uint32_t f = threadIdx.x;
    if (f >= k) return;
    const Fe r = fe_load(d_challenge, 0), lo = fe_load(fp.in[f], 0), hi = fe_load(fp.in[f], 1);
    fe_store(out, f, fe_sub(lo, fe_mul(r, fe_sub(lo, hi, P), P), P));
}

}  // namespace zk

// the completion word of host_core.hpp (host_flag_wait): the results to pinned host memory, a system-scope fence, then the word
__global__ __launch_bounds__(64) void k_publish_host(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst_host, uint32_t n_u64,
                                                     volatile uint32_t *flag, uint32_t seq) {
    // ONE wave: its lanes' stores, then one system-scope fence for the whole wave, then the word -- no workgroup barrier
    for (uint32_t i = 2 * threadIdx.x; i < n_u64; i += 2 * 64)   // n_u64 is even: elements are 4 words
        *reinterpret_cast<uint4 *>(dst_host + i) = *reinterpret_cast<const uint4 *>(src + i);
    __threadfence_system();
    if (threadIdx.x == 0) *flag = seq;
}
