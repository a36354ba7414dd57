// zerocheck.hip -- host side of the zerocheck argument (kernels: zerocheck_kernels.cuh; the context, table handles and verifier helpers
// it uses are declared in host_core.hpp).  No reference item; definition: tests/zerocheck_ref.py; DESIGN.md section 20.
//
// G(t_0[i], .., t_{k-1}[i]) = 0 on every row is proven to a verifier who afterwards needs one evaluation of every column at one point.
// The gate is a host object that carries its device program; a proof uploads it once (through pinned memory, no wait), squeezes tau on
// the device, makes every suffix's Hi and Lo table of tau with k_ml_eq_tables, and then runs per round ONE round kernel (round j >= 1:
// the fold of every column at rho_{j-1} joined to the sums) and one step kernel (partials -> g_j, absorb, rho_j).  The whole transcript
// stays on the device; the host waits once, for the published block.  Folds go out of place into two pooled blocks by turns (2^(n-1)
// and 2^(n-2) elements per column), so the caller's tables are left intact.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "zerocheck_kernels.cuh"

struct zk_gate {
    int32_t field;
    uint32_t k, T, d;
    std::vector<Fe> coeff;
    std::vector<uint32_t> len, fac;
    uint32_t prog[kZcProgWords];
};
static void gate_release(zk_gate *g) { delete g; }
enum { kZcPathProof = 0, kZcPathRound0 = 1, kZcPathRound1 = 2 };
// the call's places in the context's pinned staging (u64 words; the downloads use the front): the tail of zk_mle_gate_sums, the gate
// program with the k table pointers behind it
constexpr size_t kZcPinnedTail = 1024, kZcPinnedProg = 2048, kZcProgU64 = (kZcProgWords + 1) / 2, kZcUploadU64 = kZcProgU64 + kZcMaxCols;
static_assert(kZcPinnedProg + kZcUploadU64 <= (size_t)kMaxSums * 12, "the context's pinned staging holds the upload");
static_assert(kZcPinnedTail + 4 * kMaxVars <= kZcPinnedProg, "the tail ends in front of the program");

extern "C" int32_t zk_gate_create(int32_t field, uint32_t k, uint32_t n_terms, const uint64_t *coeffs, const uint32_t *term_len, const uint32_t *factors,
                                  zk_gate **out) {
    if (!coeffs || !term_len || !factors || !out) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    if (k < 1 || k > kZcMaxCols || n_terms < 1 || n_terms > kZcMaxTerms) return ZK_ERR_BAD_ARG;
    uint32_t mentions = 0, d = 0;
    for (uint32_t i = 0; i < n_terms; ++i) {
        if (term_len[i] > kZcMaxDegree) return ZK_ERR_BAD_ARG;
        mentions += term_len[i];
        if (term_len[i] > d) d = term_len[i];
    }
    if (mentions > kZcMaxMentions || d < 1) return ZK_ERR_BAD_ARG;
    for (uint32_t f = 0; f < mentions; ++f)
        if (factors[f] >= k) return ZK_ERR_BAD_ARG;
    zk_gate *g = new (std::nothrow) zk_gate();
    if (!g) return ZK_ERR_ALLOC;
    Scoped<zk_gate, gate_release> hold(g);
    try {
        g->coeff.resize(n_terms);
        g->len.assign(term_len, term_len + n_terms);
        g->fac.assign(factors, factors + mentions);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (uint32_t i = 0; i < n_terms; ++i)
        if (!fri_elem(coeffs + 4 * i, P, &g->coeff[i])) return ZK_ERR_BAD_ARG;
    g->field = field, g->k = k, g->T = n_terms, g->d = d;
    memset(g->prog, 0, sizeof g->prog);
    g->prog[kZcWK] = k, g->prog[kZcWT] = n_terms, g->prog[kZcWD] = d;
    const Fe one = fe_one(P), minus_one = fe_neg(one, P);
    for (uint32_t i = 0; i < n_terms; ++i) {
        const Fe &cf = g->coeff[i];
        g->prog[kZcWLen + i] = term_len[i];
        uint32_t *cw = g->prog + kZcWCoeff + 9 * i;
        if (term_len[i] == 0) {
            g->prog[kZcWKind + i] = kZcConst;
            for (int w = 0; w < 8; ++w) cw[w] = cf.v[w];
        } else if (fe_eq(cf, one) || fe_eq(cf, minus_one)) {
            g->prog[kZcWKind + i] = fe_eq(cf, one) ? kZcPlus : kZcMinus;
        } else {
            g->prog[kZcWKind + i] = kZcMul;
            const Mul29 m = mul29_prepare(cf, P);
            for (int w = 0; w < 9; ++w) cw[w] = m.l[w];
        }
    }
    for (uint32_t f = 0; f < mentions; ++f) g->prog[kZcWFactors + f] = factors[f];
    *out = hold.release();
    return ZK_OK;
}
extern "C" int32_t zk_gate_free(zk_gate *g) {
    delete g;
    return ZK_OK;
}
extern "C" int32_t zk_gate_degree(const zk_gate *g, uint32_t *out) {
    if (!g || !out) return ZK_ERR_BAD_ARG;
    *out = g->d;
    return ZK_OK;
}
extern "C" int32_t zk_gate_n_columns(const zk_gate *g, uint32_t *out) {
    if (!g || !out) return ZK_ERR_BAD_ARG;
    *out = g->k;
    return ZK_OK;
}
static uint64_t zc_proof_elems(const zk_gate *g, uint32_t n) { return (uint64_t)n * (g->d + 1) + g->k; }
extern "C" int32_t zk_zerocheck_proof_bytes(const zk_gate *g, uint32_t n_vars, uint64_t *out) {
    if (!g || !out) return ZK_ERR_BAD_ARG;
    if (n_vars < 1 || n_vars > kMaxVars) return ZK_ERR_BAD_ARG;
    *out = 32 * zc_proof_elems(g, n_vars);
    return ZK_OK;
}

// every table non-NULL (the caller has checked c, tabs and g); of this context; of one n_vars in 1 .. kMaxVars; the gate of the context's field
static int32_t zc_table_args(zk_ctx *c, const zk_mle *const *tabs, const zk_gate *g) {
    for (uint32_t i = 0; i < g->k; ++i)
        if (!tabs[i]) return ZK_ERR_BAD_ARG;
    for (uint32_t i = 0; i < g->k; ++i)
        if (tabs[i]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const uint64_t n = tabs[0]->n_vars;
    if (n < 1 || n > kMaxVars || g->field != c->field) return ZK_ERR_BAD_ARG;
    for (uint32_t i = 1; i < g->k; ++i)
        if (tabs[i]->n_vars != n) return ZK_ERR_BAD_ARG;
    return ZK_OK;
}

// the transcript's start: seed; be64(field id), be64(n), be64(k), be64(T); per term be32(c_i), be64(length), be64 per factor
static void zc_start(Sponge &sp, const zk_gate *g, uint32_t n, const uint8_t seed[32], const FieldParams &P) {
    sp.init();
    sp.update(seed, 32);
    auto be64 = [&](uint64_t v) {
        uint8_t b[8];
        for (int k = 0; k < 8; ++k) b[k] = (uint8_t)(v >> (8 * (7 - k)));
        sp.update(b, 8);
    };
    be64((uint64_t)g->field), be64(n), be64(g->k), be64(g->T);
    uint32_t f = 0;
    for (uint32_t i = 0; i < g->T; ++i) {
        uint8_t eb[32];
        fe_to_bytes_be(g->coeff[i], P, eb);
        sp.update(eb, 32);
        be64(g->len[i]);
        for (uint32_t j = 0; j < g->len[i]; ++j) be64(g->fac[f++]);
    }
}
// G at k values
static Fe zc_gate_at(const zk_gate *g, const Fe *v, const FieldParams &P) {
    Fe acc = fe_zero();
    uint32_t f = 0;
    for (uint32_t i = 0; i < g->T; ++i) {
        Fe prod = g->coeff[i];
        for (uint32_t j = 0; j < g->len[i]; ++j) prod = fe_mul(prod, v[g->fac[f++]], P);
        acc = fe_add(acc, prod, P);
    }
    return acc;
}

// ---- the device side of a proof ----------------------------------------------------------------------------------------------------
struct ZcSide {
    zk_ctx *c = nullptr;
    const zk_gate *g = nullptr;
    uint32_t n = 0, lo_max = 0;
    uint32_t *d_prog = nullptr;
    const uint64_t *const *d_cols = nullptr;
    uint64_t *hi = nullptr, *lo = nullptr, *d_tau = nullptr, *d_chal = nullptr, *buf[2] = {nullptr, nullptr};
    // T_j for j >= 1: block (j - 1) & 1, column c at c * 4 * 2^(n-j) words
    uint64_t stride_at(uint32_t j) const { return 4ull << (n - j); }
    // the blocks and the upload of the gate program and the table pointers.  with_folds = 0: round 0 only (zk_mle_gate_sums)
    int32_t init(zk_ctx *cc, const zk_mle *const *tabs, const zk_gate *gate, PoolScope &ps, bool with_folds) {
        c = cc, g = gate, n = (uint32_t)tabs[0]->n_vars;
        static bool lds_set = false;
        if (!lds_set) {
            const void *fns[4] = {reinterpret_cast<const void *>(&k_zc_round<false, false>), reinterpret_cast<const void *>(&k_zc_round<false, true>),
                                  reinterpret_cast<const void *>(&k_zc_round<true, false>), reinterpret_cast<const void *>(&k_zc_round<true, true>)};
            for (const void *f : fns) HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kZcLdsMax));
            lds_set = true;
        }
        const uint32_t nvars = n - 1;
        lo_max = nvars < kMlLoBits ? nvars : kMlLoBits;
        uint64_t *up = nullptr;
        ZKCHK(ps.get(kZcUploadU64 * 8, &up));
        ZKCHK(ps.get((size_t)64 << (nvars - lo_max), &hi));
        ZKCHK(ps.get((size_t)64 << lo_max, &lo));
        ZKCHK(ps.get((size_t)(kMaxVars + 1) * 32, &d_tau));
        ZKCHK(ps.get(kChallengeBytes, &d_chal));
        for (uint32_t j = 0; with_folds && j < 2 && j + 2 <= n; ++j) ZKCHK(ps.get((size_t)g->k * mle_block_bytes(n - 1 - j), &buf[j]));
        uint64_t *stage = c->h_pinned + kZcPinnedProg;   // pinned: the copy needs no wait
        memcpy(stage, g->prog, sizeof g->prog);
        for (uint32_t i = 0; i < g->k; ++i) stage[kZcProgU64 + i] = (uint64_t)(uintptr_t)tabs[i]->d;
        HIPCHK(hipMemcpyAsync(up, stage, (kZcProgU64 + g->k) * 8, hipMemcpyHostToDevice, c->stream));
        d_prog = reinterpret_cast<uint32_t *>(up);
        d_cols = reinterpret_cast<const uint64_t *const *>(up + kZcProgU64);
        return ZK_OK;
    }
    // every suffix's Hi and Lo table of tau_1 .. tau_{n-1}, which sit at d_tau[1 ..]
    int32_t eq_tables() {
        const uint32_t nvars = n - 1, hi_max = nvars - lo_max;
        k_ml_eq_tables<<<grid_for((2ull << hi_max) + (2ull << lo_max)), kBlock, 0, c->stream>>>(d_tau + 4, nvars, lo_max, hi, lo, c->fi->P);
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    // round j's launch: the partials land in the context's buffer, *blocks of them
    int32_t round(uint32_t j, uint32_t *blocks) {
        const FieldParams &P = c->fi->P;
        const uint32_t m = n - 1 - j, L = m < kMlLoBits ? m : kMlLoBits, k = g->k;
        ZcRound a = {};
        a.prog = d_prog;
        a.m = m;
        a.hi = hi + 4 * (1ull << (m - L)), a.lo = lo + 4 * (1ull << L);
        a.chal = d_chal;
        a.partials = c->d_partials;
        if (j <= 1) a.cols = d_cols;
        else a.src = buf[j & 1], a.src_stride = stride_at(j - 1);
        if (j >= 1) a.dst = buf[(j - 1) & 1], a.dst_stride = stride_at(j);
        uint32_t grid = 1;
        if (m >= kMlRunMinBits) {
            // a run per wave: 2^S elements, as long as the Lo table allows where that still leaves 2^kMlRunsTargetLog runs
            const uint32_t fit = m > kMlRunsTargetLog + kMlRunMinBits ? m - kMlRunsTargetLog : kMlRunMinBits, S = fit < L ? fit : L;
            const uint32_t nt = k > kZcWideCols ? kZcThreadsWide : kZcThreadsMax, wpb = nt / 64;
            const uint64_t n_runs = 1ull << (m - S), want = (n_runs + wpb - 1) / wpb;
            const size_t lds = kZcLoBytes + (size_t)k * 64 * nt;
            a.S = S;
            grid = (uint32_t)(want < kMaxGrid ? want : kMaxGrid);
            if (j) k_zc_round<true, true><<<grid, nt, lds, c->stream>>>(a, P);
            else k_zc_round<false, true><<<grid, nt, lds, c->stream>>>(a, P);
        } else {
            const size_t lds = (size_t)k * 64 * 64;
            if (j) k_zc_round<true, false><<<1, 64, lds, c->stream>>>(a, P);
            else k_zc_round<false, false><<<1, 64, lds, c->stream>>>(a, P);
        }
        HIPCHK(hipGetLastError());
        *blocks = grid;
        return ZK_OK;
    }
};

// Everything of a proof but its way to the host.  The block [n (d + 1) round elements | k final values | rho (n elements)] (Montgomery
// limbs) is left at *d_block; every block comes from the caller's scope, which outlives the queued work.  No host wait.
// upto: rounds enqueued (n: the whole proof with its finish; the bench paths stop early)
static int32_t zc_enqueue(zk_ctx *c, const zk_mle *const *tabs, const zk_gate *g, const uint8_t seed[32], PoolScope &ps, ZcSide &side, uint32_t upto,
                          uint64_t **d_block) {
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)tabs[0]->n_vars, ns = g->d + 1;
    WordSponge *d_sponge = nullptr;
    uint64_t *block = nullptr;
    ZKCHK(side.init(c, tabs, g, ps, true));
    ZKCHK(ps.get(sizeof(WordSponge), &d_sponge));
    ZKCHK(ps.get((size_t)(zc_proof_elems(g, n) + n) * 32, &block));
    Sponge sp;
    zc_start(sp, g, n, seed, P);
    ZKCHK(sponge_to_device(c, sp, d_sponge, nullptr));
    k_zc_tau<<<1, 64, 0, c->stream>>>(d_sponge, n, side.d_tau, P);
    HIPCHK(hipGetLastError());
    ZKCHK(side.eq_tables());
    uint64_t *finals = block + 4 * ((uint64_t)n * ns), *point = finals + 4 * g->k;
    for (uint32_t j = 0; j < upto; ++j) {
        uint32_t blocks = 0;
        ZKCHK(side.round(j, &blocks));
        k_zc_step<<<1, kBlock, 0, c->stream>>>(c->d_partials, blocks, ns, d_sponge, block + 4 * ((uint64_t)j * ns), point + 4 * j, side.d_chal, P);
        HIPCHK(hipGetLastError());
    }
    if (upto == n) {
        if (n == 1) k_zc_finish<<<1, 64, 0, c->stream>>>(side.d_cols, nullptr, 0, g->k, side.d_chal, finals, P);
        else k_zc_finish<<<1, 64, 0, c->stream>>>(nullptr, side.buf[(n - 2) & 1], side.stride_at(n - 1), g->k, side.d_chal, finals, P);
        HIPCHK(hipGetLastError());
    }
    *d_block = block;
    return ZK_OK;
}

extern "C" int32_t zk_zerocheck_prove(zk_ctx *c, const zk_mle *const *tabs, const zk_gate *g, const uint8_t seed[32], uint8_t *out_proof,
                                      uint64_t *out_point, uint64_t *out_claims) {
    if (!c || !tabs || !g || !seed || !out_proof || !out_point || !out_claims) return ZK_ERR_BAD_ARG;
    ZKCHK(zc_table_args(c, tabs, g));
    const FieldParams &P = c->fi->P;
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)tabs[0]->n_vars;
    const uint64_t pe = zc_proof_elems(g, n);
    const size_t bytes = (size_t)(pe + n) * 32;
    // declaration order is the order of the way out: the stream is waited for (drain) before the scratch (ps) goes back
    PoolScope ps(c);
    DrainOnExit drain(c);
    ZcSide side;
    uint64_t *d_block = nullptr;
    uint8_t *stage = nullptr;
    ZKCHK(zc_enqueue(c, tabs, g, seed, ps, side, n, &d_block));
    // the one wait of the proof: the block goes to pinned memory by a kernel that also stores the completion word
    ZKCHK(results_staging(c, bytes, &stage));
    const uint32_t seq = next_flag_seq(c);
    ZKCHK(publish_host(c, d_block, reinterpret_cast<uint64_t *>(stage), (uint32_t)(bytes / 8), seq));
    ZKCHK(host_flag_wait(c, seq));
    drain.armed = false;   // the publishing kernel was the stream's last: everything in front of it is done
    const uint64_t *h = reinterpret_cast<const uint64_t *>(stage);
    for (uint64_t i = 0; i < pe; ++i) fe_to_bytes_be(fe_from_u64limbs(h + 4 * i), P, out_proof + 32 * i);
    memcpy(out_claims, h + 4 * (pe - g->k), (size_t)g->k * 32);
    memcpy(out_point, h + 4 * pe, (size_t)n * 32);
    return ZK_OK;
}

// ---- the verifier: host only, no context; nothing sized by n ------------------------------------------------------------------------
extern "C" int32_t zk_zerocheck_verify_host(const zk_gate *g, uint32_t n_vars, const uint8_t seed[32], const uint8_t *proof, uint64_t proof_len,
                                            uint64_t *out_point, uint64_t *out_claims, int32_t *out_ok) {
    if (!g || !seed || !proof || !out_point || !out_claims || !out_ok) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(g->field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    const uint32_t n = n_vars, ns = g->d + 1;
    uint64_t want_len = 0;
    ZKCHK(zk_zerocheck_proof_bytes(g, n, &want_len));
    if (proof_len != want_len) return ZK_ERR_BAD_ARG;
    *out_ok = 0;
    for (uint64_t i = 0; i < zc_proof_elems(g, n); ++i) {
        Fe e;
        if (!fri_from_be32(proof + 32 * i, P, &e)) return ZK_OK;   // not canonical: a verdict, not an error
    }
    Sponge sp;
    zc_start(sp, g, n, seed, P);
    Fe tau[kMaxVars], rho[kMaxVars], node[kZcMaxSums], wgt[kZcMaxSums];
    for (uint32_t j = 0; j < n; ++j) tau[j] = squeeze_field_element(sp, P);
    const Fe one = fe_one(P);
    node[0] = fe_zero();
    for (uint32_t t = 1; t < ns; ++t) node[t] = fe_add(node[t - 1], one, P);
    for (uint32_t t = 0; t < ns; ++t) {   // 1 / prod_{u != t} (t - u)
        Fe den = one;
        for (uint32_t u = 0; u < ns; ++u)
            if (u != t) den = fe_mul(den, fe_sub(node[t], node[u], P), P);
        wgt[t] = fe_inverse(den, P);
    }
    Fe e = fe_zero();
    for (uint32_t j = 0; j < n; ++j) {
        const uint8_t *at = proof + 32 * ((size_t)j * ns);
        Fe gj[kZcMaxSums];
        for (uint32_t t = 0; t < ns; ++t) fri_from_be32(at + 32 * t, P, &gj[t]);
        const Fe lhs = fe_add(gj[0], fe_mul(tau[j], fe_sub(gj[1], gj[0], P), P), P);   // (1 - tau_j) g_j(0) + tau_j g_j(1)
        if (!fe_eq(lhs, e)) return ZK_OK;
        sp.update(at, (size_t)ns * 32);
        rho[j] = squeeze_field_element(sp, P);
        e = fe_zero();   // g_j(rho_j) by Lagrange on 0 .. d
        for (uint32_t t = 0; t < ns; ++t) {
            Fe term = fe_mul(gj[t], wgt[t], P);
            for (uint32_t u = 0; u < ns; ++u)
                if (u != t) term = fe_mul(term, fe_sub(rho[j], node[u], P), P);
            e = fe_add(e, term, P);
        }
    }
    Fe v[kZcMaxCols];
    const uint8_t *fin = proof + 32 * ((size_t)n * ns);
    for (uint32_t cidx = 0; cidx < g->k; ++cidx) fri_from_be32(fin + 32 * cidx, P, &v[cidx]);
    if (!fe_eq(zc_gate_at(g, v, P), e)) return ZK_OK;
    for (uint32_t j = 0; j < n; ++j) fe_to_u64limbs(rho[j], out_point + 4 * j);
    for (uint32_t cidx = 0; cidx < g->k; ++cidx) fe_to_u64limbs(v[cidx], out_claims + 4 * cidx);
    *out_ok = 1;
    return ZK_OK;
}

// ---- the sums of one round, public in its own right --------------------------------------------------------------------------------------
extern "C" int32_t zk_mle_gate_sums(zk_ctx *c, const zk_mle *const *tabs, const zk_gate *g, const uint64_t *tail, uint64_t *out) {
    if (!c || !tabs || !g || !out) return ZK_ERR_BAD_ARG;
    for (uint32_t i = 0; i < g->k; ++i)
        if (!tabs[i]) return ZK_ERR_BAD_ARG;
    if (!tail && tabs[0]->n_vars > 1) return ZK_ERR_BAD_ARG;
    ZKCHK(zc_table_args(c, tabs, g));
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)tabs[0]->n_vars, ns = g->d + 1;
    for (uint32_t j = 0; j + 1 < n; ++j) {
        Fe e;
        if (!fri_elem(tail + 4 * j, P, &e)) return ZK_ERR_BAD_ARG;
    }
    ZKCHK(use_device(c));
    PoolScope ps(c);
    DrainOnExit drain(c);
    ZcSide side;
    uint64_t *d_out = nullptr;
    ZKCHK(ps.get(kZcMaxSums * 32 + 32, &d_out));
    ZKCHK(side.init(c, tabs, g, ps, false));
    if (n > 1) {
        uint64_t *stage = c->h_pinned + kZcPinnedTail;   // pinned: the copy needs no wait
        memcpy(stage, tail, (size_t)(n - 1) * 32);
        HIPCHK(hipMemcpyAsync(side.d_tau + 4, stage, (size_t)(n - 1) * 32, hipMemcpyHostToDevice, c->stream));
    }
    ZKCHK(side.eq_tables());
    uint32_t blocks = 0;
    ZKCHK(side.round(0, &blocks));
    ZKCHK(launch_reduce_tail(c, blocks, ns, d_out));
    HIPCHK(hipMemcpyAsync(c->h_pinned, d_out, (size_t)ns * 32, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    memcpy(out, c->h_pinned, (size_t)ns * 32);
    return ZK_OK;
}

// device time of `reps` runs between two HIP events after as many untimed ones, average ms per run: path 0 = the whole proof as
// zk_zerocheck_prove enqueues it (a fixed seed; without the proof block's way to the host and its one wait), 1 = the round-0 launch
// alone, 2 = the round-1 launch alone (fold joined to the sums).  The tables are left intact.
extern "C" int32_t zk_bench_zerocheck(zk_ctx *c, const zk_mle *const *tabs, const zk_gate *g, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !tabs || !g || !out_ms || reps < 1 || path < 0 || path > 2) return ZK_ERR_BAD_ARG;
    ZKCHK(zc_table_args(c, tabs, g));
    if (path == kZcPathRound1 && tabs[0]->n_vars < 2) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const uint8_t seed[32] = {};
    if (path == kZcPathProof) {
        const uint32_t n = (uint32_t)tabs[0]->n_vars;
        DrainOnExit drain(c);
        auto once = [&]() -> int32_t {
            PoolScope ps(c);   // its blocks go back stream-ordered and come out of the pool again on the next call
            ZcSide side;
            uint64_t *d_block = nullptr;
            return zc_enqueue(c, tabs, g, seed, ps, side, n, &d_block);
        };
        ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
        drain.armed = false;   // the span has waited for ev1
        return ZK_OK;
    }
    PoolScope ps(c);
    DrainOnExit drain(c);
    ZcSide side;
    uint64_t *d_block = nullptr;
    const uint32_t j = path == kZcPathRound0 ? 0 : 1;
    ZKCHK(zc_enqueue(c, tabs, g, seed, ps, side, j, &d_block));   // the rounds in front of the timed one: tau, its tables, rho_0
    auto once = [&]() -> int32_t {
        uint32_t blocks = 0;
        return side.round(j, &blocks);
    };
    ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
    drain.armed = false;
    return ZK_OK;
}
