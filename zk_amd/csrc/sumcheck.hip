// sumcheck.hip -- the sumcheck prover's host schedule and the host verifier: which kernel closes which round (classic tail, pipelined
// launch, finisher), the single, batched and sharded provers over that one schedule, and verifier.rs restated on the host.  Kernels of
// its own: sumcheck_kernels.cuh; the round kernels are launched through launch.hpp (rounds.hip, pipe.hip).
//   sumcheck/src/prover.rs:33-73 (round loop, absorb order), sumcheck/src/verifier.rs:15-78, polynomial/src/univariate_poly.rs:29-80
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "prover_state.hpp"
#include "env.hpp"
#include "sumcheck_kernels.cuh"

// ---- round machinery ------------------------------------------------------------------------------------------
// Per-prover device scratch: the word sponge, the current challenge, and the proof being assembled.  Nothing in the
// round loop waits on the host: k_round (+fold) -> k_round_tail (reduce + transcript) -> k_round (+fold) -> ...
// The two last-block-done counters (8 bytes each) sit behind the two E-partial buffers.  A pipelined launch leaves its counter
// at zero, so they are cleared once per proof -- by the launch that stores the initial sponge (sponge_to_device), not by a
// memset of their own.
static inline uint64_t *epart_counters(uint64_t *d_epart) { return d_epart + 2 * (kEpartBytes / 8); }
// The proof being assembled is ONE device block [round polys | challenges | factor values at the point] so that it comes
// back in one copy (through pinned memory: a device-to-pageable copy blocks the host once per call).
static int32_t scratch_alloc(zk_ctx *c, ProverScratch &ps, uint64_t rounds, uint32_t D, const DeviceChain *chain = nullptr) {
    ps = ProverScratch{};
    ps.rp_bytes = (size_t)(rounds ? rounds : 1) * (D + 1) * 32;
    ps.ch_bytes = (size_t)(rounds ? rounds : 1) * 32;
    if (chain) {
        ps.external = true;
        ps.d_sponge = chain->d_sponge;
        ps.d_rp = chain->d_rp;
        ps.d_ch = chain->d_ch;
        ps.d_final = chain->d_final;
        ps.d_epart = chain->d_epart;
    } else {
        ZKCHK(ps.sponge_block.alloc(c, sizeof(WordSponge)));
        ps.d_sponge = ps.sponge_block.as<WordSponge>();
    }
    ZKCHK(ps.chal_block.alloc(c, kChalBlockBytes));
    ps.d_challenge = ps.chal_block.as();
    ps.d_claim = ps.d_challenge + 2 * kChalWords;
    if (chain) return ZK_OK;
    ZKCHK(ps.epart_block.alloc(c, kEpartBlockBytes));   // counters: cleared by sponge_to_device
    ps.d_epart = ps.epart_block.as();
    ZKCHK(ps.proof_block.alloc(c, ps.proof_block_bytes()));
    ps.d_rp = ps.proof_block.as();
    ps.d_ch = ps.d_rp + ps.rp_bytes / 8;
    ps.d_final = ps.d_ch + ps.ch_bytes / 8;
    return ZK_OK;
}

// the block partials of a round: the context's buffer -- inside a batch (launch.hpp BatchRecorder) each proof has its own eighth of it
static inline uint64_t partials_capacity() { return g_batch ? (uint64_t)kMaxGrid * kMaxSums / kMaxBatch : (uint64_t)kMaxGrid * kMaxSums; }
static inline uint64_t *partials_of(zk_ctx *c) { return g_batch ? c->d_partials + (size_t)g_batch->cur * partials_capacity() * 4 : c->d_partials; }
static inline RoundLaunchCtx launch_ctx(zk_ctx *c) {
    RoundLaunchCtx lc = {c->stream, &c->fi->P, partials_of(c), partials_capacity(), {}};
    return lc;
}
// what a launcher of launch.hpp returned (kLaunch*) as a status; `what` is the text zk_last_hip_error gives for a launch that failed
static int32_t launch_status(int lrc, const char *what) {
    if (lrc == kLaunchOk) return ZK_OK;
    g_hip_err = what;
    return lrc == kLaunchUnsupported ? ZK_ERR_UNSUPPORTED : ZK_ERR_HIP;
}
// k_round_tail on the current proof's partials: launched, or recorded for the batch's merged launch (one transcript block per proof)
static int32_t launch_tail(zk_ctx *c, uint32_t nblocks, uint32_t ns, WordSponge *sponge, uint64_t *out_rp, uint64_t *out_ch, uint64_t *d_challenge,
                           uint64_t *lanes, const TailDerive &dv, const PendingSponge *init = nullptr) {
    const uint64_t *part = partials_of(c);
    hipStream_t st = c->stream;
    const FieldParams *P = &c->fi->P;
    if (init && init->valid && sponge == init->dst && !lanes && !g_batch) {
        k_round_tail_init<<<1, kBlock, 0, st>>>(part, nblocks, ns, sponge, out_rp, out_ch, d_challenge, *P, dv, init->w, init->zero2);
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    if (init && init->valid) {   // (cannot happen with the callers as they are: the state must reach the device before anything reads it)
        k_store_sponge<<<1, 64, 0, st>>>(init->w, init->dst, init->zero2);
        HIPCHK(hipGetLastError());
    }
    auto single = [=]() {
        k_round_tail<<<1, kBlock, 0, st>>>(part, nblocks, ns, sponge, out_rp, out_ch, d_challenge, lanes, *P, dv);
        return hipGetLastError();
    };
    if (!lanes && batch_record(BK_TAIL, 0, 1, kBlock, 0, nblocks, ns, 0, 0, TailSlot{part, sponge, out_rp, out_ch, d_challenge, dv}, single)) return ZK_OK;
    HIPCHK(single());
    return ZK_OK;
}
int32_t zk::launch_reduce_tail(zk_ctx *c, uint32_t nblocks, uint32_t ns, uint64_t *out_rp) {
    k_round_tail<<<1, kBlock, 0, c->stream>>>(c->d_partials, nblocks, ns, nullptr, out_rp, nullptr, nullptr, nullptr, c->fi->P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// ZK_CLAIM_IN_ROUND=0: the tails evaluate the SKIP1 claim themselves (round 4's behaviour; A/B)
static bool claim_in_round() {
    static const bool v = env_u64("ZK_CLAIM_IN_ROUND", 1, 0, 1) != 0;
    return v;
}
static inline bool fast_degree(uint32_t D) { return D >= 1 && D <= 4; }

// Where a round's sums go after the second-stage reduction.
struct TailTargets {
    WordSponge *sponge;     // run the transcript step (single-GPU prover)
    uint64_t *out_rp;       // round polynomial, D+1 elements (device)
    uint64_t *out_ch;       // challenge record (device), may be null
    uint64_t *d_challenge;  // challenge for the next fused fold
    uint64_t *lanes;        // 32-bit digit lanes for the cross-GPU all-reduce, may be null
    const PendingSponge *init;   // non-null: the proof's initial sponge has not been stored -- this round's tail takes it as an argument
    uint64_t *claim_park;   // one element owned by the prover (ProverScratch::d_claim); null: no SKIP1 round is possible (no previous round)
    TailDerive *lanes_dv;   // with lanes (host memory, may be null): out -- what k_lanes_transcript has to derive after the all-reduce
                            // (S(1) from the claim, S(D) from the leading coefficient); null: the round kernels compute every sum
};
// value at x of the unique polynomial of degree <= D through (i, ys[i]), i = 0..D: what
// UnivariatePolynomial::interpolate(ys).evaluate(x) returns (univariate_poly.rs:43-49, :29-40); exact in F_p.
// Lagrange basis on the nodes 0..D: w_i = 1 / prod_{j != i} (i - j), computed once per proof (one field inversion each)
// Barycentric weights of the nodes 0..D: one field inversion per node (~0.1 ms of host time for D = 2), so they are computed
// once per (modulus, D) and kept (a GKR verification interpolates in 2 x depth sumchecks).
static std::vector<Fe> interp_weights_compute(uint32_t D, const FieldParams &P) {
    std::vector<Fe> w(D + 1);
    for (uint32_t i = 0; i <= D; ++i) {
        Fe den = fe_one(P);
        const Fe xi = fe_from_u32(i, P);
        for (uint32_t j = 0; j <= D; ++j)
            if (j != i) den = fe_mul(den, fe_sub(xi, fe_from_u32(j, P), P), P);
        w[i] = fe_inverse(den, P);
    }
    return w;
}
static std::vector<Fe> interp_weights(uint32_t D, const FieldParams &P) {
    static std::mutex mu;
    static std::map<std::pair<std::array<uint32_t, 8>, uint32_t>, std::vector<Fe>> cache;
    std::array<uint32_t, 8> key;
    for (int i = 0; i < 8; ++i) key[i] = P.p[i];
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({key, D});
    if (it == cache.end()) it = cache.emplace(std::make_pair(key, D), interp_weights_compute(D, P)).first;
    return it->second;
}
// Rounds with at least this many pairs leave out the t = 1 sums (k_round_kd SKIP1 + TailDerive): below it the extra
// D + 1 dependent multiplies in the tail cost more than the products they save.  ZK_SKIP1_MIN_PAIRS overrides (tests).
static uint64_t skip1_min_pairs() {
    static const uint64_t v = env_u64("ZK_SKIP1_MIN_PAIRS", (uint64_t)1 << 16, 1, (uint64_t)1 << 40);
    return v;
}
static inline TermSpec single_term(int k) {
    TermSpec ts = {1, {k, 0, 0, 0}};
    return ts;
}
// sums of the current tables (already folded) -> targets.  Handles every degree.  With several terms each term's round
// kernel writes its own range of block partials and the one tail reduction adds them all (the sum over terms is free).
// dv (optional): previous round polynomial + Lagrange weights; allows the big fused rounds to skip the t = 1 sums.
// defer (optional): when the sums take the one-launch fast path, do NOT launch k_round_tail; report what it would have
// reduced (the caller merges the tail into the next pipelined launch).  defer->blocks stays 0 when the tail was launched.
struct DeferredTail {
    uint32_t blocks;
    bool skip1;
    bool lead;    // slot D of the partials holds the leading coefficient (k_round_kd LEAD)
    const uint64_t *claim;   // skip1: where the round kernel's claim workgroup left S_prev(r_prev) (null: the tail evaluates it)
};
// Rounds with at least this many pairs accumulate the leading coefficient instead of S(D) (k_round_kd LEAD): one modular
// addition per factor and pair index fewer against three to six more in the tail.  ZK_LEAD_MIN_PAIRS overrides (tests).
static uint64_t lead_min_pairs() {
    static const uint64_t v = env_u64("ZK_LEAD_MIN_PAIRS", (uint64_t)1 << 16, 1, (uint64_t)1 << 40);
    return v;
}
// ZK_SHARD_SKIP1=0: the sharded prover's round kernels compute every sum themselves (round 4's behaviour; A/B)
static bool shard_skip_on() {
    static const bool v = env_u64("ZK_SHARD_SKIP1", 1, 0, 1) != 0;
    return v;
}
static int32_t launch_sums(zk_ctx *c, const FactorPtrs &fp, const TermSpec &ts, uint64_t q, uint32_t D, bool fused,
                           const uint64_t *d_r, const TailTargets &tt, const TailDerive *dv = nullptr, DeferredTail *defer = nullptr) {
    if (defer) defer->blocks = 0;
    const FieldParams &P = c->fi->P;
    if (fast_degree(D)) {
        uint32_t total = 0;
        int first = 0;
        // (sharded: both variants accumulate quantities that are linear in the shards, so they survive the all-reduce; the
        // derivations move behind it -- tt.lanes_dv tells zk_shard_prover_round_finish what to derive)
        const bool may_derive = !tt.lanes || (tt.lanes_dv && shard_skip_on());
        bool skip1 = dv && dv->prev_rp && tt.claim_park && fused && may_derive && D <= (uint32_t)kMaxSkipDegree && q >= skip1_min_pairs();
        bool lead = may_derive && q >= lead_min_pairs();   // (the launchers clear it for shapes without the variant)
        // a SKIP1 kernel, if one is launched below, evaluates the claim its tail needs beside its work blocks (ClaimJob)
        ClaimJob cjob = {};
        if (skip1 && claim_in_round()) cjob = ClaimJob{dv->prev_rp, dv->prev_chal, dv->w, tt.claim_park, D + 1};
        auto with_claim = [&](RoundLaunchCtx lc) {
            lc.claim = cjob;
            return lc;
        };
        auto tail_dv = [&]() {
            TailDerive t = skip1 && dv ? *dv : TailDerive{};
            t.lead = lead ? D : 0;
            t.claim = (t.prev_rp && cjob.out) ? cjob.out : nullptr;
            if (tt.lanes) {
                if (tt.lanes_dv) *tt.lanes_dv = t;
                t.local_only = 1;
            }
            return t;
        };
        if (tt.lanes_dv) *tt.lanes_dv = TailDerive{};
        bool one_pass = false;
        if (ts.n_terms == 2 && ts.term_k[1] == 1) {   // product + one single-factor term (a GKR layer): one pass
            const int lrc = launch_round_plus1(with_claim(launch_ctx(c)), fp, ts.term_k[0], q, D, fused, d_r, &total, &skip1, &lead);
            if (lrc == kLaunchHipError) return launch_status(lrc, "round kernel launch failed");
            one_pass = lrc == kLaunchOk;   // a shape without the one-pass kernel: term by term below
        }
        if (!one_pass && ts.n_terms != 1) {
            skip1 = lead = false;
            cjob = {};   // no SKIP1 kernel below: no claim workgroup either
        }
        for (int i = 0; !one_pass && i < ts.n_terms; ++i) {
            FactorPtrs sub = {};
            for (int f = 0; f < ts.term_k[i]; ++f) {
                sub.in[f] = fp.in[first + f];
                sub.out[f] = fp.out[first + f];
            }
            RoundLaunchCtx lc = with_claim(launch_ctx(c));
            lc.d_partials += (size_t)total * (D + 1) * 4;
            lc.capacity_elems -= (uint64_t)total * (D + 1);
            uint32_t g = 0;
            ZKCHK(launch_status(launch_round(lc, sub, ts.term_k[i], q, D, fused, d_r, &g, &skip1, &lead), "round kernel launch failed"));
            total += g;
            first += ts.term_k[i];
        }
        if (defer) {
            *defer = DeferredTail{total, skip1, lead, skip1 ? cjob.out : nullptr};
            return ZK_OK;
        }
        return launch_tail(c, total, D + 1, tt.sponge, tt.out_rp, tt.out_ch, tt.d_challenge, tt.lanes, tail_dv(), tt.init);
    }
    if (ts.n_terms != 1) return ZK_ERR_UNSUPPORTED;
    const int k = ts.term_k[0];
    // any other degree (0, or > 4): one pass per evaluation point over tables that are already folded
    for (uint32_t t = 0; t <= D; ++t) {
        uint32_t g = 0;
        ZKCHK(launch_status(launch_round_single_t(launch_ctx(c), fp, k, q, fe_from_u32(t, P), &g), "round kernel launch failed"));
        k_round_tail<<<1, kBlock, 0, c->stream>>>(c->d_partials, g, 1, nullptr, c->d_sums + 4 * t, nullptr, nullptr, nullptr, P);
        HIPCHK(hipGetLastError());
    }
    k_round_tail<<<1, kBlock, 0, c->stream>>>(c->d_sums, 1, D + 1, tt.sponge, tt.out_rp, tt.out_ch, tt.d_challenge, tt.lanes, P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

int32_t zk::round_sums_enqueue(zk_ctx *c, const zk_mle *const *f, uint64_t k, uint32_t D, const uint64_t **d_sums_out) {
    ZKCHK(product_args(c, f, k));
    if (D >= kMaxSums) return ZK_ERR_UNSUPPORTED;
    if (f[0]->n_vars == 0) return ZK_ERR_PANIC_INDEX;   // partial_evaluate(0, [..]) on a 0-variable poly panics
    FactorPtrs fp = {};
    for (uint64_t i = 0; i < k; ++i) fp.in[i] = f[i]->d;
    const uint64_t q = 1ull << (f[0]->n_vars - 1);
    uint64_t *d_out = c->d_sums + 4 * kMaxSums;   // second third of d_sums
    TailTargets tt = {nullptr, d_out, nullptr, nullptr, nullptr, nullptr, nullptr};
    ZKCHK(launch_sums(c, fp, single_term((int)k), q, D, false, nullptr, tt));
    *d_sums_out = d_out;
    return ZK_OK;
}
extern "C" int32_t zk_round_sums(zk_ctx *c, const zk_mle *const *f, uint64_t k, uint32_t D, uint64_t *out) {
    if (!out) return ZK_ERR_BAD_ARG;
    const uint64_t *d_out = nullptr;
    ZKCHK(round_sums_enqueue(c, f, k, D, &d_out));
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)(D + 1) * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}

static int32_t absorb_tables(zk_ctx *c, Sponge &sp, zk_mle *const *f, uint64_t k) {
    return stream_table_bytes(c, (const zk_mle *const *)f, k, [&](const uint8_t *p, size_t bytes) { sp.update(p, bytes); });
}

// ------------------------------------------------------------------------------------------------------------
// SumcheckProver -- device-resident round loop (prover.rs:33-73)
// ------------------------------------------------------------------------------------------------------------
// challenge records alternate between two slots: round s publishes into slot s & 1
static inline uint64_t *chal_of_round(const RoundState &st, uint64_t round) { return st.ps.d_challenge + (round & 1) * kChalWords; }
static inline uint64_t *chal_cur(const RoundState &st) { return chal_of_round(st, st.round); }        // this round's (to be written)
static inline uint64_t *chal_prev(const RoundState &st) { return chal_of_round(st, st.round + 1); }   // round - 1 (same parity as round + 1)
static inline uint64_t *epart_of_round(const RoundState &st, uint64_t round) { return st.ps.d_epart + (round & 1) * (kEpartBytes / 8); }
static inline uint32_t *epart_counter(const RoundState &st, uint64_t round) {
    return reinterpret_cast<uint32_t *>(st.ps.d_epart + 2 * (kEpartBytes / 8) + (round & 1));
}
// st: a default-constructed (empty) state
static int32_t round_state_init(RoundState &st, zk_ctx *c, zk_mle *const *f, uint64_t k, uint32_t D, bool consume,
                                uint64_t total_rounds, const DeviceChain *chain = nullptr) {
    st.c = c;
    st.k = k;
    st.vars_left = f[0]->n_vars;
    st.D = D;
    st.first_out_of_place = !consume;
    st.terms = single_term((int)k);
    for (uint64_t i = 0; i < k; ++i) st.cur[i] = f[i]->d;
    // (on a failure what has been allocated stays with st and goes back when the caller's RoundState dies)
    ZKCHK(scratch_alloc(c, st.ps, total_rounds, D, chain));
    if (D >= 1 && D <= (uint32_t)kMaxSkipDegree) {
        auto it = c->lagrange_w.find(D);
        if (it == c->lagrange_w.end()) {
            const std::vector<Fe> w = interp_weights(D, c->fi->P);
            std::vector<uint64_t> limbs(4 * (size_t)(D + 1));
            for (uint32_t t = 0; t <= D; ++t) fe_to_u64limbs(w[t], limbs.data() + 4 * t);
            RawBlock d_w;
            ZKCHK(raw_alloc(c, limbs.size() * 8, d_w.put()));
            HIPCHK(hipMemcpy(d_w.get(), limbs.data(), limbs.size() * 8, hipMemcpyHostToDevice));
            it = c->lagrange_w.emplace(D, static_cast<uint64_t *>(d_w.release())).first;   // the context keeps it (ctx_teardown)
        }
        st.dv.w = it->second;
    }
    if (!consume && st.vars_left >= 2)
        for (uint64_t i = 0; i < k; ++i) ZKCHK(st.scratch[i].alloc(c, (size_t)32 << (st.vars_left - 1)));
    return ZK_OK;
}
// store the proof's initial sponge with a launch of its own (what every proof did until round 6): for first transcript steps that are
// not a classic tail (a pipelined launch, a finisher) and for the batch / sharded provers
static int32_t flush_pending_sponge(RoundState &st) {
    if (!st.init.valid) return ZK_OK;
    st.init.valid = false;
    k_store_sponge<<<1, 64, 0, st.c->stream>>>(st.init.w, st.init.dst, st.init.zero2);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// Enqueue the next round: apply the pending fold (prover.rs:64 of the previous round, fused) and compute this round's
// sums (prover.rs:49-56).  `lanes` selects the sharded form (sums -> digit lanes, transcript deferred).
static int32_t round_enqueue(RoundState &st, uint64_t *lanes, DeferredTail *defer = nullptr, TailDerive *lanes_dv = nullptr) {
    zk_ctx *c = st.c;
    if (st.pending_fold) st.vars_left -= 1;           // tables shrink by the fold fused into this launch
    const uint64_t m = st.vars_left;                  // variables of this round's table
    if (m == 0) return ZK_ERR_BAD_ARG;
    const uint64_t q = 1ull << (m - 1);
    FactorPtrs fp = {};
    for (uint64_t i = 0; i < st.k; ++i) {
        fp.in[i] = st.cur[i];
        fp.out[i] = (st.pending_fold && st.first_out_of_place && st.scratch[i]) ? st.scratch[i].as() : st.cur[i];   // else in place
    }
    TailTargets tt;
    tt.sponge = lanes ? nullptr : st.ps.d_sponge;
    tt.out_rp = st.ps.d_rp + st.round * (st.D + 1) * 4;
    tt.out_ch = st.ps.d_ch + st.round * 4;
    tt.d_challenge = chal_cur(st);
    tt.lanes = lanes;
    tt.claim_park = st.ps.d_claim;
    tt.lanes_dv = lanes_dv;
    // the initial sponge, if it has not been stored yet: this round's tail takes it as an argument when it is a classic tail launched right
    // here (launch_sums on a supported degree, not deferred into a pipelined launch, not sharded); else it is stored now
    tt.init = nullptr;
    if (st.init.valid) {
        if (!lanes && !defer && fast_degree(st.D) && !st.pending_fold) tt.init = &st.init;
        else ZKCHK(flush_pending_sponge(st));
    }
    int32_t rc;
    if (st.pending_fold && !fast_degree(st.D)) {
        // generic degree: fold as separate launches, then the per-point passes
        for (uint64_t i = 0; i < st.k; ++i) {
            k_fold_dev<<<grid_for(q * 2), kBlock, 0, c->stream>>>(fp.in[i], fp.out[i], q * 2, (uint32_t)m, c->fi->P, chal_prev(st));
            HIPCHK(hipGetLastError());
        }
        FactorPtrs g = {};
        for (uint64_t i = 0; i < st.k; ++i) g.in[i] = fp.out[i];
        rc = launch_sums(c, g, st.terms, q, st.D, false, nullptr, tt);
    } else {
        st.dv.prev_rp = st.round ? tt.out_rp - (size_t)(st.D + 1) * 4 : nullptr;
        st.dv.prev_chal = chal_prev(st);
        rc = launch_sums(c, fp, st.terms, q, st.D, st.pending_fold, chal_prev(st), tt, &st.dv, defer);
        if (tt.init) st.init.valid = false;   // (consumed by the tail; on an error the proof is abandoned anyway)
    }
    if (st.pending_fold) {
        for (uint64_t i = 0; i < st.k; ++i) st.cur[i] = fp.out[i];
        st.first_out_of_place = false;
    }
    st.pending_fold = true;    // this round's challenge gets applied by the next launch
    return rc;
}

// ---- pipelined rounds (pipe_kernels.cuh): host schedule -------------------------------------------------------------------
// Rounds with at most this many pairs have their sums prepared before their challenge exists (0 switches the pipeline
// off; ZK_PIPE_MAX_PAIRS overrides; the accumulators hold at most kMaxLazy products per lane, hence the cap).
static uint64_t pipe_max_pairs() {
    static const uint64_t v = [] {
        uint64_t x = env_u64("ZK_PIPE_MAX_PAIRS", (uint64_t)1 << 12, 0, (uint64_t)1 << 40);   // 0 = no pipelined rounds; capped below
        const uint64_t cap = (uint64_t)kPipeMaxWorkBlocks * 16 * kMaxLazy;   // products a lane may accumulate unreduced (16 rows per block)
        return x > cap ? cap : x;
    }();
    return v;
}
// the state's terms as a shape of the pipelined kernels: a k-factor product (+ extra = 1: one single-factor term); ok: instantiated
struct PipeShape {
    int k, extra;
    bool ok;
};
static PipeShape pipe_shape(const RoundState &st) {
    const TermSpec &ts = st.terms;
    const bool plus1 = ts.n_terms == 2 && ts.term_k[1] == 1;
    if (ts.n_terms != 1 && !plus1) return {0, 0, false};
    return {ts.term_k[0], plus1 ? 1 : 0, pipe_shape_ok(ts.term_k[0], st.D, plus1 ? 1 : 0)};
}
static constexpr size_t kDbgWords = 64 * 32 + 64 * 16;
static uint64_t *pipe_dbg_slot(zk_ctx *c, bool finisher) {
    static const bool on = env_flag("ZK_PIPE_DEBUG");
    if (!on) return nullptr;
    if (!c->d_dbg) {
        if (hipMalloc(&c->d_dbg, kDbgWords * 8) != hipSuccess) return nullptr;
        (void)hipMemset(c->d_dbg, 0, kDbgWords * 8);
    }
    if (finisher) return c->d_dbg + 64 * 32;
    const uint32_t i = c->dbg_launch++ % 64;
    return c->d_dbg + (size_t)i * 32;
}
static void pipe_dbg_dump(zk_ctx *c) {
    if (!c->d_dbg) return;
    std::vector<uint64_t> h(kDbgWords);
    if (hipMemcpy(h.data(), c->d_dbg, kDbgWords * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    uint64_t t0 = 0;
    for (uint32_t i = 0; i < c->dbg_launch && i < 64; ++i) {
        const uint64_t *d = h.data() + (size_t)i * 32;
        if (!t0) t0 = d[0];
        fprintf(stderr, "[pipe %2u] tail: start %7.2f red %5.2f eval %5.2f transcript %5.2f publish %5.2f | work: start %7.2f loop %5.2f close %5.2f store %5.2f\n", i,
                (d[0] - t0) / 100.0, (d[1] - d[0]) / 100.0, (d[2] - d[1]) / 100.0, (d[3] - d[2]) / 100.0, (d[4] - d[3]) / 100.0,
                d[8] ? (d[8] - t0) / 100.0 : 0.0, (d[9] - d[8]) / 100.0, (d[10] - d[9]) / 100.0, (d[11] - d[10]) / 100.0);
    }
    const uint64_t *f = h.data() + 64 * 32;
    for (uint32_t r = 0; r < 24 && f[16 * r]; ++r) {
        const uint64_t *d = f + 16 * r;
        fprintf(stderr, "[fin %2u] start %7.2f gather %5.2f eval %5.2f transcript %5.2f barrier %5.2f | work %5.2f (from %5.2f)\n", r, (d[0] - t0) / 100.0,
                (d[1] - d[0]) / 100.0, (d[2] - d[1]) / 100.0, (d[3] - d[2]) / 100.0, (d[4] - d[3]) / 100.0, d[8] ? (d[9] - d[8]) / 100.0 : 0.0,
                d[8] ? (d[8] - d[0]) / 100.0 : 0.0);
    }
    (void)hipMemset(c->d_dbg, 0, kDbgWords * 8);
    c->dbg_launch = 0;
}
// the pipelined finisher takes over from every state when the tables it would hold fit LDS (ZK_FINISH_PIPE=0: classic one)
static bool finish_pipe_on() {
    static const bool v = env_u64("ZK_FINISH_PIPE", 1, 0, 1) != 0;
    return v;
}
static bool finish_pipe_applies(const RoundState &st) {
    const PipeShape s = pipe_shape(st);
    if (!finish_pipe_on() || !s.ok) return false;
    return st.vars_left >= 3 && st.vars_left - 1 <= (uint64_t)finish_pipe_max_vars(s.k + s.extra);
}
// May round (st.round + 1) be prepared by the pipeline, given that round st.round's table has m_s variables?
static bool pipe_wants_next(const RoundState &st, uint64_t m_s) {
    if (!pipe_max_pairs() || !pipe_shape(st).ok) return false;
    if (m_s < 3) return false;                                                       // the launches after it need 8 elements
    if (!finish_pipe_on() && m_s - 1 <= (uint64_t)kFinishVars) return false;          // the classic finisher takes round + 1
    return ((uint64_t)1 << (m_s - 2)) <= pipe_max_pairs();
}
// every remaining round in one launch of the pipelined finisher, from whatever state the loop is in
static int32_t finish_pipe_enqueue(RoundState &st) {
    zk_ctx *c = st.c;
    const PipeShape s = pipe_shape(st);
    FinishPipeLaunch fl = {};
    fl.k = s.k;
    fl.extra = s.extra;
    fl.D = st.D;
    fl.m_in = (uint32_t)st.vars_left;
    fl.entry = st.pipe_active ? 2 : (st.pending_fold ? 1 : 0);
    fl.e_partials = epart_of_round(st, st.round);
    fl.e_blocks = 1;   // slot 0 of the buffer holds the total ...
    if (st.pipe_active && !st.pipe_total) {   // ... unless the launch before left its block partials only (slots 1 .. pipe_blocks)
        fl.e_partials += (size_t)pipe_values_per_block(s.k, st.D) * 4;
        fl.e_blocks = st.pipe_blocks;
    }
    fl.pc = c->pipe_consts;
    fl.chal_in = chal_prev(st);
    const uint64_t remaining = st.pending_fold ? st.vars_left - 1 : st.vars_left;
    fl.chal_last = chal_of_round(st, st.round + remaining - 1);
    fl.sponge = st.ps.d_sponge;
    fl.out_rp = st.ps.d_rp + st.round * (st.D + 1) * 4;
    fl.out_ch = st.ps.d_ch + st.round * 4;
    fl.out_final = st.d_final;
    fl.dbg = pipe_dbg_slot(c, true);
    fl.pub = st.pub;
    FactorPtrs fp = {};
    for (uint64_t i = 0; i < st.k; ++i) fp.in[i] = st.cur[i];
    ZKCHK(launch_status(launch_finish_pipe(launch_ctx(c), fp, fl), "pipelined finisher launch failed"));
    st.round += remaining;
    st.vars_left = 0;
    st.pending_fold = false;
    st.pipe_active = false;
    st.published = st.pub.flag != nullptr;
    return ZK_OK;
}
static PipeTailArgs pipe_tail_args(const RoundState &st, int mode, const uint64_t *partials, uint32_t nblocks, uint32_t n_in) {
    PipeTailArgs ta = {};
    ta.dbg = pipe_dbg_slot(st.c, false);
    ta.partials = partials;
    ta.nblocks = nblocks;
    ta.n_in = n_in;
    ta.mode = mode;
    ta.chal_in = chal_prev(st);
    ta.chal_out = chal_cur(st);
    ta.sponge = st.ps.d_sponge;
    ta.out_rp = st.ps.d_rp + st.round * (st.D + 1) * 4;
    ta.out_ch = st.ps.d_ch + st.round * 4;
    ta.pc = st.c->pipe_consts;
    return ta;
}
// Classic round st.round whose sums kernel has just been launched with its tail deferred (dt): ONE launch closes it
// (transcript block) and prepares round + 1 from the table of this round (already folded: `cur`).
static int32_t pipe_enter(RoundState &st, const DeferredTail &dt) {
    zk_ctx *c = st.c;
    const PipeShape s = pipe_shape(st);
    PipeLaunch pl = {};
    pl.k = s.k;
    pl.extra = s.extra;
    pl.D = st.D;
    pl.fold = false;
    pl.emit = 1;
    pl.q = (uint64_t)1 << (st.vars_left - 2);   // vars_left = variables of this round's table (after its fold)
    pl.chal_fold = nullptr;
    pl.e_partials = epart_of_round(st, st.round + 1);
    pl.done_counter = epart_counter(st, st.round + 1);
    pl.tail = pipe_tail_args(st, 0, partials_of(c), dt.blocks, st.D + 1);
    if (dt.skip1) {
        pl.tail.dv = st.dv;
        pl.tail.dv.prev_rp = pl.tail.out_rp - (size_t)(st.D + 1) * 4;
        pl.tail.dv.prev_chal = chal_prev(st);
        pl.tail.dv.claim = dt.claim;
    }
    pl.tail.dv.lead = dt.lead ? st.D : 0;
    FactorPtrs fp = {};
    for (uint64_t i = 0; i < st.k; ++i) fp.in[i] = fp.out[i] = st.cur[i];
    uint32_t g = 0;
    ZKCHK(launch_status(launch_round_pipe(launch_ctx(c), fp, pl, &g), "pipelined round launch failed"));
    st.pipe_active = true;
    st.pipe_blocks = g;
    st.pipe_total = true;
    return ZK_OK;
}
// Pipelined state at round s = st.round: cur = table of round s-1 (vars_left variables), its challenge r_{s-1} pending, E_s
// partials ready.  ONE launch: transcript block closes round s; work blocks fold cur at r_{s-1} and, when round s+1 stays in
// the pipeline, prepare E_{s+1}.
static int32_t pipe_step(RoundState &st) {
    zk_ctx *c = st.c;
    const PipeShape s = pipe_shape(st);
    const uint64_t m = st.vars_left;             // variables of cur = table of round s - 1
    const bool stay = pipe_wants_next(st, m - 1);
    PipeLaunch pl = {};
    pl.k = s.k;
    pl.extra = s.extra;
    pl.D = st.D;
    pl.fold = true;
    pl.emit = stay ? 1 : 0;
    pl.q = m >= 3 ? (uint64_t)1 << (m - 3) : 0;
    if (pl.q == 0) return ZK_ERR_BAD_ARG;        // cannot happen: the finisher takes tables this small
    pl.chal_fold = chal_prev(st);
    pl.e_partials = epart_of_round(st, st.round + 1);
    pl.done_counter = epart_counter(st, st.round + 1);
    pl.tail = pipe_tail_args(st, 1, epart_of_round(st, st.round), 1, pipe_values_per_block(s.k, st.D));   // slot 0: the total
    if (!st.pipe_total) {   // the launch before left its block partials only: this transcript block adds them up
        pl.tail.partials = epart_of_round(st, st.round) + (size_t)pipe_values_per_block(s.k, st.D) * 4;
        pl.tail.nblocks = st.pipe_blocks;
    }
    FactorPtrs fp = {};
    for (uint64_t i = 0; i < st.k; ++i) {
        fp.in[i] = st.cur[i];
        fp.out[i] = (st.first_out_of_place && st.scratch[i]) ? st.scratch[i].as() : st.cur[i];
    }
    uint32_t g = 0;
    ZKCHK(launch_status(launch_round_pipe(launch_ctx(c), fp, pl, &g), "pipelined round launch failed"));
    for (uint64_t i = 0; i < st.k; ++i) st.cur[i] = fp.out[i];
    st.first_out_of_place = false;
    st.vars_left = m - 1;                        // cur = table of round s, r_s pending
    st.pipe_active = stay;
    st.pipe_blocks = g;
    st.pipe_total = true;
    ++st.round;
    return ZK_OK;
}

// ---- finisher: every remaining round in one single-workgroup launch (k_finish) ----
// dynamic LDS of k_finish / k_finish_terms, as the kernels carve it: k tables of 2^m elements (m_in variables, one fewer after a pending
// fold), the waves' partial sums, the D + 1 sums, the challenge
static size_t finish_lds_bytes(uint64_t k, uint32_t D, uint32_t m_in, int pending) {
    const uint32_t m = pending ? m_in - 1 : m_in;
    return (size_t)k * ((size_t)32 << m) + (kBlock / 64) * (D + 1) * 32 + (D + 1) * 32 + 48;
}
template <int K, int D>
static int32_t launch_finish(zk_ctx *c, const FactorPtrs &fp, uint32_t m_in, int pending, uint64_t *d_challenge, WordSponge *sp,
                             uint64_t *out_rp, uint64_t *out_ch, uint64_t *out_final) {
    const size_t lds = finish_lds_bytes(K, D, m_in, pending);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_finish<K, D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipStream_t st = c->stream;
    const FieldParams *P = &c->fi->P;
    auto single = [=]() {
        k_finish<K, D><<<1, kBlock, lds, st>>>(fp, m_in, pending, *P, d_challenge, sp, out_rp, out_ch, out_final);
        return hipGetLastError();
    };
    if (batch_record_other(single)) return ZK_OK;   // (no batched twin: a batch replays the classic finisher proof by proof)
    HIPCHK(single());
    return ZK_OK;
}
// the (k, D) shapes k_finish is instantiated for
#define ZK_FINISH_SHAPES(X) X(1, 1) X(1, 2) X(2, 1) X(2, 2) X(2, 3) X(3, 2) X(3, 3)
static bool finish_shape_ok(uint64_t k, uint32_t D) {
#define ZK_SHAPE_IS(K, DD) \
    if (k == K && D == DD) return true;
    ZK_FINISH_SHAPES(ZK_SHAPE_IS)
#undef ZK_SHAPE_IS
    return false;
}
// Runs rounds st.round .. (st.round + remaining - 1) where remaining = variables left after the pending fold.
static int32_t finish_enqueue(RoundState &st) {
    zk_ctx *c = st.c;
    FactorPtrs fp = {};
    for (uint64_t i = 0; i < st.k; ++i) fp.in[i] = st.cur[i];
    const int pending = st.pending_fold ? 1 : 0;
    const uint32_t m_in = (uint32_t)st.vars_left;
    const uint64_t remaining = pending ? st.vars_left - 1 : st.vars_left;
    uint64_t *out_rp = st.ps.d_rp + st.round * (st.D + 1) * 4, *out_ch = st.ps.d_ch + st.round * 4;
    int32_t rc = ZK_ERR_UNSUPPORTED;
    if (st.terms.n_terms > 1) {
        const size_t lds = finish_lds_bytes(st.k, st.D, m_in, pending);
        const FieldParams &P = c->fi->P;
#define ZK_FINISH_TERMS(DD)                                                                                                     \
    case DD:                                                                                                                    \
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_finish_terms<DD>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                (int)lds) != hipSuccess)                                                                        \
            return ZK_ERR_HIP;                                                                                                  \
        k_finish_terms<DD><<<1, kBlock, lds, c->stream>>>(fp, st.terms, m_in, pending, P, chal_prev(st), st.ps.d_sponge,     \
                                                          out_rp, out_ch, st.d_final);                                          \
        break;
        switch (st.D) {
            ZK_FINISH_TERMS(1)
            ZK_FINISH_TERMS(2)
            ZK_FINISH_TERMS(3)
            ZK_FINISH_TERMS(4)
            default: return ZK_ERR_UNSUPPORTED;
        }
#undef ZK_FINISH_TERMS
        rc = hipGetLastError() == hipSuccess ? ZK_OK : ZK_ERR_HIP;
    } else {
#define ZK_FINISH(K, DD) \
    if (st.k == K && st.D == DD) rc = launch_finish<K, DD>(c, fp, m_in, pending, chal_prev(st), st.ps.d_sponge, out_rp, out_ch, st.d_final);
        ZK_FINISH_SHAPES(ZK_FINISH)
#undef ZK_FINISH
    }
    if (rc == ZK_OK) {
        st.round += remaining;
        st.vars_left = 0;
        st.pending_fold = false;
    }
    return rc;
}
static inline bool finish_applies(const RoundState &st) {
    if (st.terms.n_terms == 1 ? !finish_shape_ok(st.k, st.D) : !fast_degree(st.D)) return false;
    const uint64_t after = st.pending_fold ? st.vars_left - 1 : st.vars_left;
    return after >= 1 && after <= (uint64_t)kFinishVars;
}

// One step of the single-GPU round loop (prover.rs:44-68): everything that can be enqueued for round st.round.
static int32_t prover_step(RoundState &st, bool *finished_in_kernel) {
    if (st.init.valid && (finish_pipe_applies(st) || st.pipe_active || finish_applies(st))) ZKCHK(flush_pending_sponge(st));
    if (finish_pipe_applies(st)) {                                       // (covers the pipelined state as well)
        *finished_in_kernel = true;
        return finish_pipe_enqueue(st);
    }
    if (st.pipe_active) return pipe_step(st);
    if (finish_applies(st)) {
        *finished_in_kernel = true;
        return finish_enqueue(st);                                       // all remaining rounds in one launch
    }
    // the table of this round has m_s variables; if the NEXT round belongs to the pipeline, this round's tail is merged
    // into the launch that prepares it
    const uint64_t m_s = st.pending_fold ? st.vars_left - 1 : st.vars_left;
    DeferredTail dt = {0, false, false, nullptr};
    const bool enter = fast_degree(st.D) && pipe_wants_next(st, m_s);
    ZKCHK(round_enqueue(st, nullptr, enter ? &dt : nullptr));
    // dt.blocks == 0: round_enqueue's contract for "the tail was launched after all" (a sums path that cannot defer it) --
    // the round is closed and its challenge published, so the next round simply takes the classic path
    if (enter && dt.blocks) ZKCHK(pipe_enter(st, dt));
    ++st.round;
    return ZK_OK;
}

// host byte sponge (table + claimed sum absorbed) -> device word sponge.  The 208-byte state travels as a kernel argument:
// no staging buffer, no copy engine, no host synchronisation in front of the first round.
// d_epart: the E-partial block whose two counters the same launch clears (every proof starts with this launch)
int32_t zk::sponge_to_device(zk_ctx *c, const Sponge &host, WordSponge *d_sponge, uint64_t *d_epart) {
    WordSponge w;
    if (!w.from_byte_sponge(host)) return ZK_ERR_BAD_ARG;
    uint64_t *zero2 = d_epart ? epart_counters(d_epart) : nullptr;
    hipStream_t st = c->stream;
    auto single = [=]() {
        k_store_sponge<<<1, 64, 0, st>>>(w, d_sponge, zero2);
        return hipGetLastError();
    };
    if (batch_record(BK_STORE_SPONGE, 0, 1, 64, 0, 0, 0, 0, 0, SpongeSlot{w, d_sponge, zero2}, single)) return ZK_OK;
    HIPCHK(single());
    return ZK_OK;
}
// k_publish_host as a call for the other units (gprod.hip): n_u64 words of a device block into pinned host memory, then the completion word
int32_t zk::publish_host(zk_ctx *c, const uint64_t *d_src, uint64_t *h_dst, uint32_t n_u64, uint32_t seq) {
    k_publish_host<<<1, 64, 0, c->stream>>>(d_src, h_dst, n_u64, c->h_flag, seq);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// ZK_SPONGE_IN_TAIL=0: the initial sponge goes to the device with a launch of its own in front of round 0 (until round 6; A/B)
static bool sponge_in_tail() {
    static const bool v = env_u64("ZK_SPONGE_IN_TAIL", 1, 0, 1) != 0;
    return v;
}
// ZK_PUBLISH_IN_FINISHER=0: the proof block always goes to pinned host memory by k_publish_host, never by the pipelined finisher (A/B)
static bool publish_in_finisher() {
    static const bool v = env_u64("ZK_PUBLISH_IN_FINISHER", 1, 0, 1) != 0;
    return v;
}

static bool has_duplicate_handles(zk_mle *const *f, uint64_t k) {
    for (uint64_t i = 0; i < k; ++i)
        for (uint64_t j = i + 1; j < k; ++j)
            if (f[i] == f[j]) return true;
    return false;
}
// The prover for sum_i prod_{f in term i} T_f (one term = the reference's ProductPoly).  out_final (optional): the k
// factors evaluated at the challenge point.
// d_keep_ch / d_keep_final (optional, DEVICE buffers of n / k elements): device-resident copies of the challenges and of the
// factor values, for a caller that chains further device work on them without a host round trip (the GKR driver).
int32_t zk::prove_core(zk_ctx *c, zk_mle *const *f, uint64_t k, const TermSpec &ts, uint32_t D, const uint64_t sum[4],
                          int32_t absorb_table, int32_t consume, uint64_t *out_rp, uint64_t *out_ch, uint64_t *out_final,
                          uint64_t *d_keep_ch, uint64_t *d_keep_final, const Sponge *init, const DeviceChain *chain) {
    if (!sum && !chain) return ZK_ERR_BAD_ARG;
    ZKCHK(product_args(c, (const zk_mle *const *)f, k));
    if (chain) {   // device-resident transcript: enqueue the rounds and return (no host data, no synchronisation)
        const uint64_t n = f[0]->n_vars;
        if (n == 0 || D >= kMaxSums) return ZK_ERR_UNSUPPORTED;
        if (has_duplicate_handles(f, k)) consume = 0;
        RoundState st;   // its scratch goes back to the pool when the call returns: stream-ordered reuse
        ZKCHK(round_state_init(st, c, f, k, D, consume != 0, n, chain));
        st.terms = ts;
        st.d_final = st.ps.d_final;
        bool fin = false;
        while (st.round < n) ZKCHK(prover_step(st, &fin));
        if (!fin) {
            FactorPtrs fp = {};
            for (uint64_t i = 0; i < k; ++i) fp.in[i] = st.cur[i];
            k_final_evals<<<1, 64, 0, c->stream>>>(fp, (uint32_t)k, chal_prev(st), st.d_final, c->fi->P);
            HIPCHK(hipGetLastError());
        }
        return ZK_OK;
    }
    if (f[0]->n_vars && (!out_rp || !out_ch)) return ZK_ERR_BAD_ARG;
    if (D >= kMaxSums) return ZK_ERR_UNSUPPORTED;
    const FieldParams &P = c->fi->P;
    const uint64_t n = f[0]->n_vars;
    Sponge sp;
    if (init) sp = *init;                                                // a driver chaining its sumchecks onto its own transcript (GKR)
    else sp.init();                                                      // Transcript::new (prover.rs:16,28)
    if (absorb_table) ZKCHK(absorb_tables(c, sp, f, k));                 // prover.rs:17
    absorb_elements(sp, sum, 1, P);                                      // prover.rs:42
    if (n == 0) {                                                        // no rounds (prover.rs:44)
        if (out_final)
            for (uint64_t i = 0; i < k; ++i) ZKCHK(zk_mle_download(c, f[i], out_final + 4 * i));
        return ZK_OK;
    }
    // the reference takes the polynomial by value and clones per fold, so a table may appear twice (A * A): in-place folds
    // would then fold the shared buffer once per listing -- such a product is proved out of place (own scratch per factor)
    if (has_duplicate_handles(f, k)) consume = 0;
    static const bool host_dbg = env_flag("ZK_HOST_DEBUG");
    const auto t_enter = std::chrono::steady_clock::now();
    RoundState st;
    ZKCHK(round_state_init(st, c, f, k, D, consume != 0, n));
    st.terms = ts;
    if (out_final) st.d_final = st.ps.d_final;
    uint8_t *stage = nullptr;
    const size_t block = st.ps.proof_block_bytes();
    uint32_t seq = 0;
    // everything up to the last launch; a failure in it waits for the stream below before the scratch goes back
    auto enqueue = [&]() -> int32_t {
        if (sponge_in_tail() && !g_batch) {
            if (!st.init.w.from_byte_sponge(sp)) return ZK_ERR_BAD_ARG;
            st.init.dst = st.ps.d_sponge;
            st.init.zero2 = st.ps.d_epart ? epart_counters(st.ps.d_epart) : nullptr;
            st.init.valid = true;
        } else {
            ZKCHK(sponge_to_device(c, sp, st.ps.d_sponge, st.ps.d_epart));
        }
        // one copy of [round polys | challenges | finals] into pinned memory behind a completion word: by the pipelined finisher itself
        // when it is the call's last launch (publish_in_finisher), else by k_publish_host below
        ZKCHK(results_staging(c, block, &stage));
        seq = next_flag_seq(c);
        if (publish_in_finisher() && !d_keep_ch && !d_keep_final)
            st.pub = FinishPublish{st.ps.d_rp, reinterpret_cast<uint64_t *>(stage), (uint32_t)(block / 8), c->h_flag, seq};
        bool finished_in_kernel = false;
        while (st.round < n) ZKCHK(prover_step(st, &finished_in_kernel));   // prover.rs:44-68, all on device
        // prover.rs:64 after the LAST round folds to a 0-variable polynomial the reference drops: computed only on request.
        if (out_final && !finished_in_kernel) {
            FactorPtrs fp = {};
            for (uint64_t i = 0; i < k; ++i) fp.in[i] = st.cur[i];
            k_final_evals<<<1, 64, 0, c->stream>>>(fp, (uint32_t)k, chal_prev(st), st.d_final, P);
            HIPCHK(hipGetLastError());
        }
        if (d_keep_ch) HIPCHK(hipMemcpyAsync(d_keep_ch, st.ps.d_ch, (size_t)n * 32, hipMemcpyDeviceToDevice, c->stream));
        if (d_keep_final && out_final) HIPCHK(hipMemcpyAsync(d_keep_final, st.ps.d_final, (size_t)k * 32, hipMemcpyDeviceToDevice, c->stream));
        if (!st.published) {   // the proof block goes to pinned memory by a kernel that also stores the completion word
            k_publish_host<<<1, 64, 0, c->stream>>>(st.ps.d_rp, reinterpret_cast<uint64_t *>(stage), (uint32_t)(block / 8), c->h_flag, seq);
            HIPCHK(hipGetLastError());
        }
        return ZK_OK;
    };
    // rc is kept from here on: the wait, the debug output and the dump run after a failure too
    int32_t rc = enqueue();
    const auto t_enq = std::chrono::steady_clock::now();
    if (rc == ZK_OK) rc = host_flag_wait(c, seq);
    else (void)stream_wait(c->stream);
    if (host_dbg) {
        const auto t_done = std::chrono::steady_clock::now();
        fprintf(stderr, "[host] n=%llu: enqueue %.1f us (everything up to the last launch), wait %.1f us\n", (unsigned long long)n,
                std::chrono::duration<double, std::micro>(t_enq - t_enter).count(), std::chrono::duration<double, std::micro>(t_done - t_enq).count());
    }
    if (c->d_dbg) pipe_dbg_dump(c);
    if (rc == ZK_OK) {
        memcpy(out_rp, stage, (size_t)n * (D + 1) * 32);
        memcpy(out_ch, stage + st.ps.rp_bytes, (size_t)n * 32);
        if (out_final) memcpy(out_final, stage + st.ps.rp_bytes + st.ps.ch_bytes, (size_t)k * 32);
    }
    return rc;
}

extern "C" int32_t zk_sumcheck_prove(zk_ctx *c, zk_mle *const *f, uint64_t k, uint32_t D, const uint64_t sum[4],
                                     int32_t absorb_table, int32_t consume, uint64_t *out_rp, uint64_t *out_ch) {
    if (k == 0 || k > (uint64_t)kMaxFactors) return product_args(c, (const zk_mle *const *)f, k);
    return prove_core(c, f, k, single_term((int)k), D, sum, absorb_table, consume, out_rp, out_ch, nullptr);
}

// prove_partial for a SUM of products (what a GKR layer needs): factors flat, term_k[i] factors per term.
// Tables must not be shared between terms (each is folded by the term that lists it).
extern "C" int32_t zk_sumcheck_prove_terms(zk_ctx *c, zk_mle *const *f, const uint64_t *term_k, uint64_t n_terms, uint32_t D,
                                           const uint64_t sum[4], int32_t consume, uint64_t *out_rp, uint64_t *out_ch,
                                           uint64_t *out_final) {
    if (!c || !f || !term_k) return ZK_ERR_BAD_ARG;
    if (n_terms == 0) return ZK_ERR_EMPTY_PRODUCT;
    if (n_terms > (uint64_t)kMaxTerms) return ZK_ERR_UNSUPPORTED;
    TermSpec ts = {};
    ts.n_terms = (int)n_terms;
    uint64_t k = 0;
    for (uint64_t i = 0; i < n_terms; ++i) {
        if (term_k[i] == 0) return ZK_ERR_EMPTY_PRODUCT;
        if (term_k[i] > (uint64_t)kMaxFactors || term_k[i] > D) return ZK_ERR_UNSUPPORTED;   // a term of k factors has degree k
        ts.term_k[i] = (int)term_k[i];
        k += term_k[i];
    }
    if (k > (uint64_t)kMaxFactors) return ZK_ERR_UNSUPPORTED;
    for (uint64_t i = 0; i < k; ++i)
        for (uint64_t j = i + 1; j < k; ++j)
            if (f[i] && f[i] == f[j]) return ZK_ERR_BAD_ARG;
    if (n_terms > 1 && !fast_degree(D)) return ZK_ERR_UNSUPPORTED;
    return prove_core(c, f, k, ts, D, sum, 0, consume, out_rp, out_ch, out_final);
}

extern "C" int32_t zk_sumcheck_prove_host(zk_ctx *c, const uint64_t *const *tables, uint64_t k, uint64_t n_vars, uint32_t D,
                                          const uint64_t sum[4], int32_t absorb_table, uint64_t *out_rp, uint64_t *out_ch) {
    if (!c) return ZK_ERR_BAD_ARG;
    if (k == 0) return ZK_ERR_EMPTY_PRODUCT;
    if (!tables || k > (uint64_t)kMaxFactors) return tables ? ZK_ERR_UNSUPPORTED : ZK_ERR_BAD_ARG;
    MleHolder own[kMaxFactors];
    zk_mle *h[kMaxFactors] = {};
    for (uint64_t i = 0; i < k; ++i) {
        ZKCHK(zk_mle_upload(c, n_vars, tables[i], 1ull << n_vars, own[i].put()));
        h[i] = own[i].get();
    }
    return zk_sumcheck_prove(c, h, k, D, sum, absorb_table, 1, out_rp, out_ch);
}

// ------------------------------------------------------------------------------------------------------------
// B independent proofs in ONE launch sequence (config 4 as SURVEY 8d words it: "8 independent layers x (k = 3, n = 20)")
// ------------------------------------------------------------------------------------------------------------
// n_proofs separate prove_partial calls (prover.rs:24-30: one per ProductPoly; nothing in the reference orders independent calls) of
// one shape (k, D) and one size, each with its own transcript, proved side by side: the host schedule of a proof runs once per proof
// with a recorder installed (launch.hpp), and launch i of all proofs is issued as one launch of the kernel's batched twin -- the B
// transcript steps of a round run next to each other instead of one after the other, and the number of launches does not grow with B.
// Every proof is bit-identical to the one zk_sumcheck_prove returns for the same inputs (same kernels' bodies, same arithmetic).
static thread_local uint64_t g_batch_merged = 0, g_batch_replayed = 0;
static int32_t batch_flush(BatchRecorder &r) {
    int32_t rc = ZK_OK;   // a chain: after a failure nothing more is launched, but every proof's record list is still cleared
    const size_t len = r.recs[0].size();
    bool same_len = true;
    for (int b = 1; b < r.n; ++b) same_len = same_len && r.recs[b].size() == len;
    auto replay = [&](int b, size_t i) {
        if (rc == ZK_OK && r.recs[b][i].single() != hipSuccess) {
            g_hip_err = "batched prover: a replayed launch failed";
            rc = ZK_ERR_HIP;
        }
        ++r.replayed;
    };
    if (!same_len) {   // cannot happen for proofs of one shape and size; proofs are independent, so proof-by-proof order is valid too
        for (int b = 0; b < r.n; ++b)
            for (size_t i = 0; i < r.recs[b].size(); ++i) replay(b, i);
    } else {
        for (size_t i = 0; i < len && rc == ZK_OK; ++i) {
            const BatchRecord &r0 = r.recs[0][i];
            bool same = r0.kernel != BK_OTHER;
            for (int b = 1; b < r.n && same; ++b) {
                const BatchRecord &x = r.recs[b][i];
                same = x.kernel == r0.kernel && x.shape == r0.shape && x.grid == r0.grid && x.block == r0.block && x.lds == r0.lds &&
                       memcmp(x.s, r0.s, sizeof r0.s) == 0;
            }
            int lrc = kLaunchUnsupported;
            if (same) {
                const dim3 grid(r0.grid, (uint32_t)r.n);
                if (r0.kernel == BK_STORE_SPONGE) {
                    BatchOf<SpongeSlot> slots;
                    batch_gather(r, i, slots);
                    k_store_sponge_b<<<grid, r0.block, 0, r.stream>>>(slots);
                    lrc = hipGetLastError() == hipSuccess ? kLaunchOk : kLaunchHipError;
                } else if (r0.kernel == BK_TAIL) {
                    BatchOf<TailSlot> slots;
                    batch_gather(r, i, slots);
                    k_round_tail_b<<<grid, r0.block, 0, r.stream>>>(slots, (uint32_t)r0.s[0], (uint32_t)r0.s[1], *r.P);
                    lrc = hipGetLastError() == hipSuccess ? kLaunchOk : kLaunchHipError;
                } else if (r0.kernel == BK_PIPE || r0.kernel == BK_FINISH_PIPE) {
                    lrc = batch_launch_pipe(r, i);
                } else {
                    lrc = batch_launch_rounds(r, i);
                }
            }
            if (lrc == kLaunchOk) {
                ++r.merged;
            } else if (lrc == kLaunchHipError) {
                g_hip_err = "batched prover: a merged launch failed";
                rc = ZK_ERR_HIP;
            } else {
                static const bool dbg = env_flag("ZK_BATCH_DEBUG");
                if (dbg)
                    fprintf(stderr, "[batch] step %zu replayed: kernel %d shape 0x%x grid %u block %u lds %zu s = %llu %llu %llu %llu (%s)\n", i, r0.kernel,
                            r0.shape, r0.grid, r0.block, r0.lds, (unsigned long long)r0.s[0], (unsigned long long)r0.s[1], (unsigned long long)r0.s[2],
                            (unsigned long long)r0.s[3], same ? "no batched twin" : "shared arguments differ between the proofs");
                for (int b = 0; b < r.n; ++b) replay(b, i);
            }
        }
    }
    for (int b = 0; b < r.n; ++b) r.recs[b].clear();
    return rc;
}
// up to kMaxBatch proofs; f = B * k handles (proof-major), sums = B * 4 words, outputs proof-major
static int32_t prove_batch_group(zk_ctx *c, int B, zk_mle *const *f, uint64_t k, uint32_t D, const uint64_t *sums, int32_t consume, uint64_t *out_rp,
                                 uint64_t *out_ch) {
    const uint64_t n = f[0]->n_vars;
    const size_t rp_words = (size_t)n * (D + 1) * 4, ch_words = (size_t)n * 4;
    if (B == 1 || n == 0 || !fast_degree(D)) {   // nothing to merge, or a degree whose rounds go through context-wide scratch: one by one
        for (int b = 0; b < B; ++b)
            ZKCHK(prove_core(c, f + (size_t)b * k, k, single_term((int)k), D, sums + 4 * b, 0, consume, out_rp + b * rp_words, out_ch + b * ch_words, nullptr));
        return ZK_OK;
    }
    const FieldParams &P = c->fi->P;
    BatchRecorder rec;
    rec.n = B;
    rec.stream = c->stream;
    rec.P = &P;
    struct Guard {   // the recorder is installed for this thread only while the schedule runs
        explicit Guard(BatchRecorder *r) { g_batch = r; }
        ~Guard() { g_batch = nullptr; }
    };
    std::vector<RoundState> st((size_t)B);   // each proof's scratch goes back when the group returns
    // an rc chain: after a failure the schedule stops, but the recorder's statistics are still published and the stream is still
    // waited for before the scratch goes back
    int32_t rc = ZK_OK;
    uint32_t seq[kMaxBatch] = {};
    uint8_t *stage = nullptr;
    size_t block = 0;
    {
        Guard guard(&rec);
        for (int b = 0; b < B && rc == ZK_OK; ++b) {
            rec.cur = b;
            rc = round_state_init(st[(size_t)b], c, f + (size_t)b * k, k, D, consume != 0, n);
        }
        if (rc == ZK_OK) {
            block = (st[0].ps.proof_block_bytes() + 63) & ~(size_t)63;
            rc = results_staging(c, block * (size_t)B, &stage);
        }
        for (int b = 0; b < B && rc == ZK_OK; ++b) {
            rec.cur = b;
            RoundState &s = st[(size_t)b];
            s.terms = single_term((int)k);
            Sponge sp;
            sp.init();                                        // Transcript::new (prover.rs:28)
            absorb_elements(sp, sums + 4 * b, 1, P);          // prover.rs:42
            rc = sponge_to_device(c, sp, s.ps.d_sponge, s.ps.d_epart);
            seq[b] = next_flag_seq(c);
            if (publish_in_finisher())
                s.pub = FinishPublish{s.ps.d_rp, reinterpret_cast<uint64_t *>(stage + block * (size_t)b), (uint32_t)(block / 8), c->h_flag + 16 * b, seq[b]};
        }
        if (rc == ZK_OK) rc = batch_flush(rec);
        while (rc == ZK_OK && st[0].round < n) {              // prover.rs:44-68: one step of every proof, then the merged launches
            for (int b = 0; b < B && rc == ZK_OK; ++b) {
                rec.cur = b;
                bool fin = false;
                rc = prover_step(st[(size_t)b], &fin);
            }
            if (rc == ZK_OK) rc = batch_flush(rec);
        }
        for (int b = 0; b < B && rc == ZK_OK; ++b) {
            rec.cur = b;
            RoundState &s = st[(size_t)b];
            if (s.round != n) rc = ZK_ERR_BAD_ARG;            // (the proofs must have advanced in lockstep)
            if (rc == ZK_OK && !s.published) {
                const uint64_t *src = s.ps.d_rp;
                uint64_t *dst = reinterpret_cast<uint64_t *>(stage + block * (size_t)b);
                const uint32_t words = (uint32_t)(s.ps.proof_block_bytes() / 8);
                volatile uint32_t *flag = c->h_flag + 16 * b;
                const uint32_t sq = seq[b];
                hipStream_t stream = c->stream;
                (void)batch_record_other([=]() {
                    k_publish_host<<<1, 64, 0, stream>>>(src, dst, words, flag, sq);
                    return hipGetLastError();
                });
            }
        }
        if (rc == ZK_OK) rc = batch_flush(rec);
    }
    g_batch_merged = rec.merged;
    g_batch_replayed = rec.replayed;
    for (int b = 0; b < B; ++b) {
        if (rc == ZK_OK) rc = host_flag_wait(c, seq[b], (uint32_t)b);
    }
    if (rc != ZK_OK) (void)stream_wait(c->stream);
    if (rc == ZK_OK) {
        for (int b = 0; b < B; ++b) {
            const uint8_t *src = stage + block * (size_t)b;
            memcpy(out_rp + b * rp_words, src, rp_words * 8);
            memcpy(out_ch + b * ch_words, src + st[(size_t)b].ps.rp_bytes, ch_words * 8);
        }
    }
    return rc;
}
static int32_t prove_batch_impl(zk_ctx *c, uint64_t n_proofs, zk_mle *const *f, uint64_t k, uint32_t D, const uint64_t *sums, int32_t consume,
                                uint64_t *out_rp, uint64_t *out_ch) {
    if (!c || !f || !sums) return ZK_ERR_BAD_ARG;
    if (n_proofs == 0) return ZK_OK;
    if (k == 0) return ZK_ERR_EMPTY_PRODUCT;
    if (k > (uint64_t)kMaxFactors || D >= kMaxSums) return ZK_ERR_UNSUPPORTED;
    for (uint64_t p = 0; p < n_proofs; ++p) {
        ZKCHK(product_args(c, (const zk_mle *const *)(f + p * k), k));          // each proof: ProductPoly::new's checks (product_poly.rs:14-32)
        if (f[p * k]->n_vars != f[0]->n_vars) return ZK_ERR_ARITY_MISMATCH;      // a batch is one size
    }
    const uint64_t n = f[0]->n_vars;
    if (n && (!out_rp || !out_ch)) return ZK_ERR_BAD_ARG;
    // in-place folds need every table to be its proof's own: a handle listed twice (inside a proof, or by two proofs) -> out of place
    if (consume) {
        std::set<const zk_mle *> seen;
        for (uint64_t i = 0; i < n_proofs * k && consume; ++i)
            if (!seen.insert(f[i]).second) consume = 0;
    }
    g_batch_merged = g_batch_replayed = 0;
    uint64_t merged = 0, replayed = 0;
    const size_t rp_words = (size_t)n * (D + 1) * 4, ch_words = (size_t)n * 4;
    for (uint64_t p0 = 0; p0 < n_proofs; p0 += kMaxBatch) {
        const int B = (int)std::min<uint64_t>(kMaxBatch, n_proofs - p0);
        ZKCHK(prove_batch_group(c, B, f + p0 * k, k, D, sums + 4 * p0, consume, out_rp ? out_rp + p0 * rp_words : nullptr,
                                out_ch ? out_ch + p0 * ch_words : nullptr));
        merged += g_batch_merged;
        replayed += g_batch_replayed;
    }
    g_batch_merged = merged;
    g_batch_replayed = replayed;
    return ZK_OK;
}
// the recorder keeps its launches in host containers: an allocation failure is a status, never an exception across the C ABI
extern "C" int32_t zk_sumcheck_prove_batch(zk_ctx *c, uint64_t n_proofs, zk_mle *const *f, uint64_t k, uint32_t D, const uint64_t *sums, int32_t consume,
                                           uint64_t *out_rp, uint64_t *out_ch) {
    try {
        return prove_batch_impl(c, n_proofs, f, k, D, sums, consume, out_rp, out_ch);
    } catch (const std::bad_alloc &) {   // (the recorder's guard has uninstalled it during the unwinding)
        if (c) (void)stream_wait(c->stream);
        return ZK_ERR_ALLOC;
    } catch (...) {
        if (c) (void)stream_wait(c->stream);
        return ZK_ERR_BAD_ARG;
    }
}
// what the last zk_sumcheck_prove_batch of this thread did: launches issued for all proofs at once / replayed proof by proof
extern "C" int32_t zk_batch_last_stats(uint64_t *out_merged, uint64_t *out_replayed) {
    if (!out_merged || !out_replayed) return ZK_ERR_BAD_ARG;
    *out_merged = g_batch_merged;
    *out_replayed = g_batch_replayed;
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// sharded prover: the same loop with one exchange point per round
// ------------------------------------------------------------------------------------------------------------
static void shard_prover_delete(zk_shard_prover *sp) { delete sp; }
extern "C" int32_t zk_shard_prover_create(zk_ctx *c, zk_mle *const *f, uint64_t k, uint32_t D, const uint64_t sum[4],
                                          uint32_t world, zk_shard_prover **out) {
    if (!out || !sum) return ZK_ERR_BAD_ARG;
    ZKCHK(product_args(c, (const zk_mle *const *)f, k));
    if (D >= kMaxSums) return ZK_ERR_UNSUPPORTED;
    if (world == 0 || (world & (world - 1)) || world > 65536) return ZK_ERR_BAD_ARG;
    zk_shard_prover *sp = new (std::nothrow) zk_shard_prover();
    if (!sp) return ZK_ERR_ALLOC;
    sp->world = world;
    sp->local_rounds = f[0]->n_vars;
    sp->total_rounds = f[0]->n_vars + log2_world(world);
    Scoped<zk_shard_prover, shard_prover_delete> owner(sp);
    // the shard tables are consumed (folded in place) unless one is listed twice (see prove_core)
    ZKCHK(round_state_init(sp->st, c, f, k, D, /*consume=*/!has_duplicate_handles(f, k), sp->total_rounds));
    ZKCHK(sp->lanes.alloc(c, (size_t)kMaxSums * 8 * sizeof(uint64_t)));
    Sponge host;
    host.init();
    absorb_elements(host, sum, 1, c->fi->P);   // prover.rs:42 -- the GLOBAL claimed sum, identical on every rank
    ZKCHK(sponge_to_device(c, host, sp->st.ps.d_sponge, sp->st.ps.d_epart));
    *out = owner.release();
    return ZK_OK;
}
extern "C" int32_t zk_shard_prover_destroy(zk_shard_prover *sp) {
    if (!sp) return ZK_OK;
    (void)hipSetDevice(sp->st.c->device);
    delete sp;   // its members give their blocks back
    return ZK_OK;
}
extern "C" int32_t zk_shard_prover_lanes_ptr(zk_shard_prover *sp, void **out_ptr, uint64_t *out_n) {
    if (!sp || !out_ptr || !out_n) return ZK_ERR_BAD_ARG;
    *out_ptr = sp->lanes.p;
    *out_n = (uint64_t)(sp->st.D + 1) * 8;
    return ZK_OK;
}
extern "C" int32_t zk_shard_prover_rounds(zk_shard_prover *sp, uint64_t *out_local, uint64_t *out_total, uint64_t *out_done) {
    if (!sp) return ZK_ERR_BAD_ARG;
    if (out_local) *out_local = sp->local_rounds;
    if (out_total) *out_total = sp->total_rounds;
    if (out_done) *out_done = sp->st.round;
    return ZK_OK;
}
// local part of a round: (fold +) sums -> digit lanes.  Asynchronous.
extern "C" int32_t zk_shard_prover_round_begin(zk_shard_prover *sp) {
    if (!sp) return ZK_ERR_BAD_ARG;
    RoundState &st = sp->st;
    if (st.round >= sp->local_rounds) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(st.c));
    sp->lanes_dv = TailDerive{};
    return round_enqueue(st, sp->lanes.as(), nullptr, &sp->lanes_dv);
}
// after the caller's all-reduce of the lanes: reduce mod p, absorb, squeeze.  Asynchronous.
extern "C" int32_t zk_shard_prover_round_finish(zk_shard_prover *sp) {
    if (!sp) return ZK_ERR_BAD_ARG;
    RoundState &st = sp->st;
    zk_ctx *c = st.c;
    if (st.round >= sp->local_rounds || !st.pending_fold) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    sp->lanes_dv.log_world = log2_world(sp->world);
    k_lanes_transcript<<<1, 128, 0, c->stream>>>(sp->lanes.as(), st.D + 1, st.ps.d_sponge, st.ps.d_rp + st.round * (st.D + 1) * 4,
                                                st.ps.d_ch + st.round * 4, chal_cur(st), c->fi->P, sp->lanes_dv);
    HIPCHK(hipGetLastError());
    ++st.round;
    return ZK_OK;
}
// Stop exchanging per round: apply the pending challenge and expose this rank's k shard tables (2^s elements each,
// s = local variables still unfolded; s = 0 after the last local round) as one device buffer [k][2^s] for the all-gather.
// May be called after any number of local rounds: once shards are tiny a collective per round costs more than finishing
// redundantly on every rank.
extern "C" int32_t zk_shard_prover_tail_ptr(zk_shard_prover *sp, void **out_ptr, uint64_t *out_elems) {
    if (!sp || !out_ptr || !out_elems) return ZK_ERR_BAD_ARG;
    RoundState &st = sp->st;
    zk_ctx *c = st.c;
    if (st.round > sp->local_rounds) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    if (!sp->tail_done) {
        const uint64_t s = st.pending_fold ? st.vars_left - 1 : st.vars_left;
        sp->tail_s = (uint32_t)s;
        ZKCHK(sp->tail.alloc(c, (size_t)st.k * ((size_t)32 << s)));
        for (uint64_t i = 0; i < st.k; ++i) {
            uint64_t *dst = sp->tail.as() + ((uint64_t)i << s) * 4;
            if (st.pending_fold) {
                const uint64_t pairs = 1ull << s;
                k_fold_dev<<<grid_for(pairs), kBlock, 0, c->stream>>>(st.cur[i], dst, pairs, (uint32_t)(s + 1), c->fi->P, chal_prev(st));
                HIPCHK(hipGetLastError());
            } else {
                HIPCHK(hipMemcpyAsync(dst, st.cur[i], (size_t)32 << s, hipMemcpyDeviceToDevice, c->stream));
            }
        }
        st.pending_fold = false;
        st.vars_left = s;
        sp->tail_done = true;
    }
    *out_ptr = sp->tail.p;
    *out_elems = (uint64_t)st.k << sp->tail_s;
    return ZK_OK;
}
// gathered: device array [world][k][2^s] elements (rank-major, the all-gather of every rank's tail buffer), identical
// on every rank.  Builds the k tables of s + log2(world) variables -- global index = local * world + rank, i.e. the
// reference's own index order -- and runs ALL remaining rounds locally (no further collective).  Asynchronous.
extern "C" int32_t zk_shard_prover_tail_rounds(zk_shard_prover *sp, const void *gathered) {
    if (!sp || !gathered) return ZK_ERR_BAD_ARG;
    RoundState &st = sp->st;
    zk_ctx *c = st.c;
    if (!sp->tail_done) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const uint64_t vars = (uint64_t)sp->tail_s + log2_world(sp->world);
    if (st.round + vars != sp->total_rounds) return ZK_ERR_BAD_ARG;
    if (vars == 0) return ZK_OK;
    FactorPtrs fp = {};
    for (uint64_t i = 0; i < st.k; ++i) {
        ZKCHK(st.scratch[i].alloc(c, (size_t)32 << vars));   // (gives the previous block back first)
        fp.out[i] = st.cur[i] = st.scratch[i].as();
    }
    const uint64_t items = ((uint64_t)st.k << sp->tail_s) * sp->world;
    k_gather_to_tables<<<grid_for(items), kBlock, 0, c->stream>>>((const uint64_t *)gathered, fp, (uint32_t)st.k, sp->world, sp->tail_s);
    HIPCHK(hipGetLastError());
    st.pending_fold = false;
    st.first_out_of_place = false;
    st.vars_left = vars;
    bool fin = false;
    while (st.round < sp->total_rounds) ZKCHK(prover_step(st, &fin));
    return ZK_OK;
}
// download what has been proven so far (synchronises): total_rounds*(D+1) and total_rounds elements
extern "C" int32_t zk_shard_prover_results(zk_shard_prover *sp, uint64_t *out_rp, uint64_t *out_ch) {
    if (!sp || !out_rp || !out_ch) return ZK_ERR_BAD_ARG;
    RoundState &st = sp->st;
    zk_ctx *c = st.c;
    ZKCHK(use_device(c));
    if (st.round) {
        HIPCHK(hipMemcpyAsync(out_rp, st.ps.d_rp, (size_t)st.round * (st.D + 1) * 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(out_ch, st.ps.d_ch, (size_t)st.round * 32, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// SumcheckVerifier (host protocol logic; verifier.rs:15-78, univariate_poly.rs:29-80)
// ------------------------------------------------------------------------------------------------------------
static Fe interp_eval(const std::vector<Fe> &ys, const std::vector<Fe> &w, const Fe &x, const FieldParams &P) {
    const size_t n = ys.size();
    Fe acc = fe_zero();
    for (size_t i = 0; i < n; ++i) {
        Fe num = fe_one(P);
        for (size_t j = 0; j < n; ++j)
            if (j != i) num = fe_mul(num, fe_sub(x, fe_from_u32((uint32_t)j, P), P), P);
        acc = fe_add(acc, fe_mul(ys[i], fe_mul(num, w[i], P), P), P);
    }
    return acc;
}
// Each round polynomial is interpolated at ITS OWN length (proof.round_polys is a Vec<Vec<F>>; verifier.rs:55-58 hands
// whatever the round carries to UnivariatePolynomial::interpolate): lens[r] evaluations for round r, stored back to back.
// 0 evaluations -> the zero polynomial (interpolate of no points, evaluate of no coefficients = 0), 1 -> a constant.
// lens == nullptr: every round carries `uniform_len` evaluations (the D + 1 of verify / verify_partial) -- no per-round array is
// built from a caller-supplied round count, so a hostile count cannot make the library allocate (or throw) before it is checked.
int32_t zk::verify_internal(const FieldParams &P, Sponge &sp, uint64_t n_rounds, const uint32_t *lens, uint32_t uniform_len,
                               const uint64_t sum[4], const uint64_t *rps, Fe &claimed, uint64_t *out_ch) {   // verifier.rs:44-78
    absorb_elements(sp, sum, 1, P);                                      // :50
    claimed = fe_from_u64limbs(sum);
    std::vector<Fe> w;
    uint32_t w_len = ~0u;
    const uint64_t *rp = rps;
    for (uint64_t r = 0; r < n_rounds; ++r) {
        const uint32_t len = lens ? lens[r] : uniform_len;
        if (len) absorb_elements(sp, rp, len, P);                        // :56 (no bytes for an empty round polynomial)
        std::vector<Fe> ys(len);
        for (uint32_t t = 0; t < len; ++t) ys[t] = fe_from_u64limbs(rp + 4 * t);
        if (len && len != w_len) w = interp_weights(len - 1, P), w_len = len;
        // :61-62 p(0), p(1): the interpolant through (i, ys[i]) takes exactly ys[0], ys[1] at the nodes 0 and 1
        const Fe p0 = len ? ys[0] : fe_zero(), p1 = len >= 2 ? ys[1] : (len ? ys[0] : fe_zero());
        if (!fe_eq(claimed, fe_add(p0, p1, P))) return ZK_ERR_VERIFY_SUM;                  // :64
        const Fe ch = squeeze_field_element(sp, P);                      // :69
        claimed = len ? interp_eval(ys, w, ch, P) : fe_zero();           // :70
        fe_to_u64limbs(ch, out_ch + 4 * r);
        rp += (size_t)len * 4;
    }
    return ZK_OK;
}
int32_t zk::verify_internal(const FieldParams &P, Sponge &sp, uint64_t n_rounds, uint32_t D, const uint64_t sum[4],
                               const uint64_t *rps, Fe &claimed, uint64_t *out_ch) {   // every round D + 1 evaluations
    return verify_internal(P, sp, n_rounds, nullptr, D + 1, sum, rps, claimed, out_ch);
}
static int32_t check_lens(uint64_t n_rounds, const uint32_t *lens) {
    for (uint64_t r = 0; r < n_rounds; ++r)
        if (lens[r] > kMaxSums) return ZK_ERR_BAD_ARG;
    return ZK_OK;
}
// shared bodies of the four verifier entry points: lens == nullptr means `uniform_len` evaluations in every round
static int32_t verify_partial_common(int32_t field, uint64_t n_rounds, const uint32_t *lens, uint32_t uniform_len,
                                     const uint64_t sum[4], const uint64_t *rps, uint64_t out_sum[4], uint64_t *out_ch) {
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    if (!sum || !out_sum || (n_rounds && (!rps || !out_ch))) return ZK_ERR_BAD_ARG;
    if (lens) ZKCHK(check_lens(n_rounds, lens));
    Sponge sp;
    sp.init();
    Fe claimed;
    ZKCHK(verify_internal(fi->P, sp, n_rounds, lens, uniform_len, sum, rps, claimed, out_ch));
    fe_to_u64limbs(claimed, out_sum);
    return ZK_OK;
}
static int32_t verify_common(zk_ctx *c, const zk_mle *const *f, uint64_t k, uint64_t n_rps, const uint32_t *lens,
                             uint32_t uniform_len, const uint64_t sum[4], const uint64_t *rps, int32_t *out_ok) {
    if (!sum || !out_ok || (n_rps && !rps)) return ZK_ERR_BAD_ARG;
    ZKCHK(product_args(c, f, k));
    if (n_rps != f[0]->n_vars) return ZK_ERR_VERIFY_ROUNDS;              // verifier.rs:17-19 -- BEFORE anything is sized by n_rps
    if (lens) ZKCHK(check_lens(n_rps, lens));
    Sponge sp;
    sp.init();
    ZKCHK(absorb_tables(c, sp, (zk_mle *const *)f, k));                  // :22
    uint64_t ch[4 * (kMaxVars + 1)];                                     // n_rps == n_vars <= kMaxVars
    Fe claimed;
    ZKCHK(verify_internal(c->fi->P, sp, n_rps, lens, uniform_len, sum, rps, claimed, ch));
    uint64_t ev[4];
    ZKCHK(zk_product_evaluate(c, f, k, ch, n_rps, ev));                  // :27-29
    *out_ok = fe_eq(fe_from_u64limbs(ev), claimed) ? 1 : 0;              // :31
    return ZK_OK;
}
extern "C" int32_t zk_sumcheck_verify_partial_lengths(int32_t field, uint64_t n_rounds, const uint32_t *lens,
                                                      const uint64_t sum[4], const uint64_t *rps, uint64_t out_sum[4],
                                                      uint64_t *out_ch) {
    if (n_rounds && !lens) return ZK_ERR_BAD_ARG;
    static const uint32_t none = 0;
    return verify_partial_common(field, n_rounds, lens ? lens : &none, 0, sum, rps, out_sum, out_ch);
}
extern "C" int32_t zk_sumcheck_verify_partial(int32_t field, uint64_t n_rounds, uint32_t D, const uint64_t sum[4],
                                              const uint64_t *rps, uint64_t out_sum[4], uint64_t *out_ch) {
    if (D >= kMaxSums) return ZK_ERR_BAD_ARG;
    return verify_partial_common(field, n_rounds, nullptr, D + 1, sum, rps, out_sum, out_ch);
}
extern "C" int32_t zk_sumcheck_verify_lengths(zk_ctx *c, const zk_mle *const *f, uint64_t k, uint64_t n_rps,
                                              const uint32_t *lens, const uint64_t sum[4], const uint64_t *rps,
                                              int32_t *out_ok) {
    if (n_rps && !lens) return ZK_ERR_BAD_ARG;
    static const uint32_t none = 0;
    return verify_common(c, f, k, n_rps, lens ? lens : &none, 0, sum, rps, out_ok);
}
extern "C" int32_t zk_sumcheck_verify(zk_ctx *c, const zk_mle *const *f, uint64_t k, uint64_t n_rps, uint32_t D,
                                      const uint64_t sum[4], const uint64_t *rps, int32_t *out_ok) {
    if (D >= kMaxSums) return ZK_ERR_BAD_ARG;
    return verify_common(c, f, k, n_rps, nullptr, D + 1, sum, rps, out_ok);
}

// ------------------------------------------------------------------------------------------------------------
// measurement hook
// ------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_bench_prove_partial(zk_ctx *c, zk_mle *const *f, uint64_t k, uint32_t D, const uint64_t sum[4], int32_t reps,
                                          double *out_ms_each) {
    if (!c || !f || !sum || !out_ms_each || reps <= 0) return ZK_ERR_BAD_ARG;
    ZKCHK(product_args(c, (const zk_mle *const *)f, k));
    const uint64_t n = f[0]->n_vars;
    std::vector<uint64_t> rp((size_t)(n ? n : 1) * (D + 1) * 4), ch((size_t)(n ? n : 1) * 4);
    return wall_clock_each(c, reps, [&] { return zk_sumcheck_prove(c, f, k, D, sum, 0, 0, rp.data(), ch.data()); }, out_ms_each);
}
