// mlpcs.hip -- host side of the multilinear polynomial commitment (kernels in mlpcs_kernels.cuh; no reference item, definition:
// tests/mlpcs_ref.py): BaseFold over the FRI layers.  The commitment handle (a copy of the table, the LDE of its
// coefficient form, that layer's tree in FRI's row layout), the opening at a point (per round one codeword fold, one tree, one sumcheck
// launch and one download of the root with the round's sums; the host transcript; fri.hip's gather for the queries) and the host-only
// verifier.  The sumcheck of t(x) eq(x, z) has two routes behind ZK_MLPCS_ROUND that give the same bytes: the round kernel of
// mlpcs_kernels.cuh (no eq table, the fold of T joined to the sums), and zk_eq_table with zk_round_sums' and zk_mle_fold_into's launches.
// The shapes, the proof's length and the sumcheck's host arithmetic are ml_host.hpp's, shared with mlbatch.hip.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "ml_host.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "mlpcs_kernels.cuh"

// ZK_MLPCS_ROUND: 1 = fused (k_ml_round), 0 = tables (an eq table, the two-table round sums and two folds per round).  The default is
// what profiles/mlpcs.log shows faster at n = 24 by more than the run-to-run spread.
constexpr uint32_t kMlRoundDefault = 1;
static bool mlpcs_fused_round() {
    static const bool fused = env_u64("ZK_MLPCS_ROUND", kMlRoundDefault, 0, 1) != 0;
    return fused;
}
enum { kMlPathDefault = 0, kMlPathFused = 1, kMlPathTables = 2 };
constexpr size_t kMlPinnedPoint = 1024;   // the point's place in the context's pinned staging (u64 words; the downloads use the front)

struct zk_mlpcs {
    zk_ctx *ctx;
    uint32_t n, b;
    Fe shift;
    PoolBlock table;   // t, 2^n elements: the sumcheck's T_0, never written
    PoolBlock lde;     // F_0, 2^(n+b) elements; the tree's two columns are its halves
    PoolBlock tree;    // every level over M_0 = 2^(n+b-1) rows of two columns
};
static void mlpcs_release(zk_mlpcs *h) { delete h; }   // the blocks go back to the pool with their owner
using MlpcsHolder = Scoped<zk_mlpcs, mlpcs_release>;
using FoldPlanHolder = Scoped<FriFoldPlan, fri_fold_plan_release>;

// ---- the sumcheck side of an opening: T_0 = the committed table (read only), T_r (r >= 1) in two blocks by turns ----------------------
struct RoundSide {
    zk_ctx *c = nullptr;
    uint32_t n = 0;
    bool fused = true;
    const uint64_t *t0 = nullptr;
    PoolBlock tbuf[2], ebuf[2];   // T_r and (tables) E_r for r >= 1: block (r - 1) & 1
    MleHolder e0;                 // tables: eq(., z)
    PoolBlock d_vars, hi, lo;     // fused: z_1 .. z_{n-1} and every suffix's Hi and Lo table
    uint32_t lo_max = 0;
    uint32_t sums() const { return fused ? 2 : 3; }   // elements a round leaves: S_0, S_1 or h(0), h(1), h(2)
    const uint64_t *t_at(uint32_t r) const { return r == 0 ? t0 : tbuf[(r - 1) & 1].as(); }
    // point: n elements (Montgomery limbs, host).  Enqueues (the tables route waits once for its point, as zk_eq_table does)
    int32_t init(zk_ctx *cc, const uint64_t *table, uint32_t n_vars, const uint64_t *point, bool use_fused) {
        c = cc, n = n_vars, fused = use_fused, t0 = table;
        for (uint32_t j = 0; j < 2 && j + 2 <= n; ++j) {
            ZKCHK(tbuf[j].alloc(c, mle_block_bytes(n - 1 - j)));
            if (!fused) ZKCHK(ebuf[j].alloc(c, mle_block_bytes(n - 1 - j)));
        }
        if (!fused) return zk_eq_table(c, point, n, e0.put());
        const uint32_t nvars = n - 1;
        lo_max = nvars < kMlLoBits ? nvars : kMlLoBits;
        const uint32_t hi_max = nvars - lo_max;
        ZKCHK(d_vars.alloc(c, ml_scratch_bytes((size_t)nvars * 32)));
        ZKCHK(hi.alloc(c, (size_t)64 << hi_max));
        ZKCHK(lo.alloc(c, (size_t)64 << lo_max));
        if (nvars) {
            uint64_t *stage = c->h_pinned + kMlPinnedPoint;   // pinned: the copy needs no wait
            memcpy(stage, point + 4, (size_t)nvars * 32);
            HIPCHK(hipMemcpyAsync(d_vars.p, stage, (size_t)nvars * 32, hipMemcpyHostToDevice, c->stream));
        }
        k_ml_eq_tables<<<grid_for((2ull << hi_max) + (2ull << lo_max)), kBlock, 0, c->stream>>>(d_vars.as(), nvars, lo_max, hi.as(), lo.as(), c->fi->P);
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    // round r: (r >= 1: T_r = the fold of T_{r-1} at beta) and the round's sums of T_r -> d_out (sums() elements).  Enqueues only.
    int32_t round(uint32_t r, const Fe &beta, uint64_t *d_out) {
        const FieldParams &P = c->fi->P;
        const uint32_t m = n - r - 1;
        if (fused) {
            const uint32_t L = m < kMlLoBits ? m : kMlLoBits;
            const uint64_t *hi_r = hi.as() + 4 * (1ull << (m - L)), *lo_r = lo.as() + 4 * (1ull << L);
            const uint64_t *src = t_at(r ? r - 1 : 0);
            uint64_t *dst = r ? tbuf[(r - 1) & 1].as() : nullptr;
            const Mul29 b29 = mul29_prepare(beta, P);
            uint32_t g = 1;
            if (m >= kMlRunMinBits) {
                // a run per wave: 2^S elements, as long as the Lo table allows where that still leaves 2^kMlRunsTargetLog runs
                const uint32_t fit = m > kMlRunsTargetLog + kMlRunMinBits ? m - kMlRunsTargetLog : kMlRunMinBits, S = fit < L ? fit : L;
                const uint64_t n_runs = 1ull << (m - S), want = (n_runs + kBlock / 64 - 1) / (kBlock / 64);
                g = (uint32_t)(want < kMaxGrid ? want : kMaxGrid);
                if (r) k_ml_round<true, true><<<g, kBlock, 0, c->stream>>>(src, dst, m, S, hi_r, lo_r, b29, c->d_partials, P);
                else k_ml_round<false, true><<<g, kBlock, 0, c->stream>>>(src, dst, m, S, hi_r, lo_r, b29, c->d_partials, P);
            } else {
                if (r) k_ml_round<true, false><<<1, kBlock, 0, c->stream>>>(src, dst, m, 0, hi_r, lo_r, b29, c->d_partials, P);
                else k_ml_round<false, false><<<1, kBlock, 0, c->stream>>>(src, dst, m, 0, hi_r, lo_r, b29, c->d_partials, P);
            }
            HIPCHK(hipGetLastError());
            return launch_reduce_tail(c, g, 2, d_out);
        }
        if (r) {
            uint64_t bl[4];
            fe_to_u64limbs(beta, bl);
            const zk_mle t_in = {c, n - r + 1, const_cast<uint64_t *>(t_at(r - 1))}, e_in = {c, n - r + 1, r == 1 ? e0->d : ebuf[r & 1].as()};
            zk_mle t_out = {c, n - r, tbuf[(r - 1) & 1].as()}, e_out = {c, n - r, ebuf[(r - 1) & 1].as()};
            ZKCHK(zk_mle_fold_into(c, &t_in, bl, &t_out));
            ZKCHK(zk_mle_fold_into(c, &e_in, bl, &e_out));
        }
        const zk_mle tv = {c, n - r, const_cast<uint64_t *>(t_at(r))}, ev = {c, n - r, r ? ebuf[(r - 1) & 1].as() : e0->d};
        const zk_mle *both[2] = {&tv, &ev};
        const uint64_t *d_sums = nullptr;
        ZKCHK(round_sums_enqueue(c, both, 2, 2, &d_sums));
        HIPCHK(hipMemcpyAsync(d_out, d_sums, 96, hipMemcpyDeviceToDevice, c->stream));
        return ZK_OK;
    }
};

// ---- the commitment ------------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_mlpcs_commit(zk_ctx *c, const zk_mle *table, uint32_t log_blowup, const uint64_t shift[4], zk_mlpcs **out) {
    if (!c || !table || !shift || !out) return ZK_ERR_BAD_ARG;
    if (table->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)table->n_vars, b = log_blowup;
    Fe s;
    if (table->n_vars < 1 || table->n_vars > kMaxVars || b < 1 || b > kMlMaxBlowupLog || !fri_elem(shift, P, &s) || fe_is_zero(s)) return ZK_ERR_BAD_ARG;
    const uint32_t n0 = n + b, m = n0 - 1;
    if (n0 > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    if (n0 > kMaxVars) return ZK_ERR_UNSUPPORTED;   // layer 0 is a table like any other
    ZKCHK(use_device(c));
    MlpcsHolder h(new (std::nothrow) zk_mlpcs());
    if (!h.get()) return ZK_ERR_ALLOC;
    h->ctx = c, h->n = n, h->b = b, h->shift = s;
    PoolBlock coeffs;
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the blocks go back
    ZKCHK(h->table.alloc(c, mle_block_bytes(n)));
    ZKCHK(h->lde.alloc(c, mle_block_bytes(n0)));
    ZKCHK(h->tree.alloc(c, (size_t)64 << m));
    ZKCHK(coeffs.alloc(c, mle_block_bytes(n)));
    HIPCHK(hipMemcpyAsync(h->table.p, table->d, mle_block_bytes(n), hipMemcpyDeviceToDevice, c->stream));
    ZKCHK(cmle_interpolate_into(c, table, coeffs.as()));   // key bit v <-> variable v: coefficient j of the univariate polynomial
    const zk_upoly poly = {c, 1ull << n, coeffs.as()};
    zk_mle layer0 = {c, n0, h->lde.as()};
    ZKCHK(fri_lde_into(c, &poly, n0, shift, &layer0));
    const uint64_t *cols[2] = {h->lde.as(), h->lde.as() + 4 * (1ull << m)};
    ZKCHK(merkle_build_raw(c, cols, 2, m, h->tree.as()));
    drain.armed = false;   // enqueued: the coefficients go back stream-ordered
    *out = h.release();
    return ZK_OK;
}
extern "C" int32_t zk_mlpcs_free(zk_mlpcs *h) {
    mlpcs_release(h);   // back to its context's pool; reuse is stream-ordered
    return ZK_OK;
}
extern "C" int32_t zk_mlpcs_n_vars(const zk_mlpcs *h, uint32_t *out) {
    if (!h || !out) return ZK_ERR_BAD_ARG;
    *out = h->n;
    return ZK_OK;
}
extern "C" int32_t zk_mlpcs_root(zk_ctx *c, const zk_mlpcs *h, uint8_t out[32]) {
    if (!c || !h || !out) return ZK_ERR_BAD_ARG;
    if (h->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    const uint32_t m = h->n + h->b - 1;
    HIPCHK(hipMemcpyAsync(out, h->tree.as() + 4 * ((2ull << m) - 2), 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
extern "C" int32_t zk_mlpcs_proof_bytes(uint32_t n_vars, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries, uint64_t *out) {
    if (!out) return ZK_ERR_BAD_ARG;
    if (!ml_open_shape(n_vars, log_blowup, log_final, n_queries)) return ZK_ERR_BAD_ARG;
    *out = ml_proof_bytes(n_vars, log_blowup, log_final, n_queries);
    return ZK_OK;
}

// ---- the opening ---------------------------------------------------------------------------------------------------------------------
// One host wait per round: behind the codeword's fold r - 1 -> r, tree r and the sumcheck launch of round r, one download brings root_r
// and the round's sums (round 0: the commitment's root and the sums of t itself, of which v = (1 - z_0) S_0 + z_0 S_1 comes for free).
extern "C" int32_t zk_mlpcs_open(zk_ctx *c, const zk_mlpcs *h, const uint64_t *point, uint64_t n_point, uint32_t log_final, uint32_t n_queries,
                                 const uint8_t seed[32], uint64_t out_value[4], uint8_t *out_proof) {
    if (!c || !h || !point || !seed || !out_value || !out_proof) return ZK_ERR_BAD_ARG;
    if (h->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (n_point != h->n) return ZK_ERR_EVAL_ARITY;
    const FieldParams &P = c->fi->P;
    const uint32_t n = h->n, b = h->b, f = log_final, Q = n_queries, n0 = n + b;
    if (!ml_open_shape(n, b, f, Q)) return ZK_ERR_BAD_ARG;
    const uint32_t R = n - f;
    std::vector<Fe> z, betas;
    std::vector<MleHolder> layers;   // layers[r], r >= 1 (layer 0 is the commitment's)
    std::vector<const uint64_t *> layer_at, tree_at;
    std::vector<PoolBlock> trees;    // trees[r], r >= 1
    std::vector<uint64_t> idx, staged;
    std::vector<uint8_t> proof;
    try {
        z.resize(n);
        betas.resize(R);
        layers.resize(R + 1);
        layer_at.resize(R + 1);
        tree_at.resize(R);
        trees.resize(R);
        idx.resize(Q);
        proof.resize(ml_proof_bytes(n, b, f, Q));
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (uint32_t j = 0; j < n; ++j)
        if (!fri_elem(point + 4 * j, P, &z[j])) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    // owners first, the drain last: a call that leaves early waits for the stream before any block goes back
    RoundSide side;
    FoldPlanHolder plan;
    PoolBlock d_dl, d_idx, d_stage;
    MleHolder coeffs;
    DrainOnExit drain(c);
    ZKCHK(side.init(c, h->table.as(), n, point, mlpcs_fused_round()));
    ZKCHK(fri_fold_plan(c, n0, plan.put()));
    ZKCHK(d_dl.alloc(c, 128));   // root_r | the round's sums
    layer_at[0] = h->lde.as();
    tree_at[0] = h->tree.as();
    const uint32_t ns = side.sums();
    Sponge sp;
    Fe s_inv = fe_inverse(h->shift, P), scale = fe_one(P), value = fe_zero();
    uint8_t *at = proof.data();
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t nr = n0 - r, m = nr - 1;
        if (r) {
            ZKCHK(mle_alloc(c, nr, layers[r].put()));
            layer_at[r] = layers[r]->d;
            ZKCHK(fri_fold2(c, plan.get(), layer_at[r - 1], nr + 1, r - 1, s_inv, betas[r - 1], layers[r]->d));
            s_inv = fe_sqr(s_inv, P);
            ZKCHK(trees[r].alloc(c, (size_t)64 << m));
            const uint64_t *cols[2] = {layer_at[r], layer_at[r] + 4 * (1ull << m)};
            ZKCHK(merkle_build_raw(c, cols, 2, m, trees[r].as()));
            tree_at[r] = trees[r].as();
        }
        ZKCHK(side.round(r, r ? betas[r - 1] : fe_zero(), d_dl.as() + 4));
        HIPCHK(hipMemcpyAsync(d_dl.p, tree_at[r] + 4 * ((2ull << m) - 2), 32, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->h_pinned, d_dl.p, (size_t)(1 + ns) * 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));   // the round's one host wait
        const uint8_t *root = reinterpret_cast<const uint8_t *>(c->h_pinned);
        Fe hr[3];
        if (side.fused) ml_round_poly(fe_from_u64limbs(c->h_pinned + 4), fe_from_u64limbs(c->h_pinned + 8), scale, z[r], P, hr);
        else
            for (int t = 0; t < 3; ++t) hr[t] = fe_from_u64limbs(c->h_pinned + 4 + 4 * t);
        if (r == 0) {   // the transcript starts once the root and v are here
            value = fe_add(hr[0], hr[1], P);
            sp.init();
            sp.update(seed, 32);
            const uint64_t v[5] = {(uint64_t)c->field, n, b, f, Q};
            uint8_t be[40], eb[32];
            for (int i = 0; i < 5; ++i)
                for (int k = 0; k < 8; ++k) be[8 * i + k] = (uint8_t)(v[i] >> (8 * (7 - k)));
            sp.update(be, 40);
            fe_to_bytes_be(h->shift, P, eb);
            sp.update(eb, 32);
            sp.update(root, 32);
            for (uint32_t j = 0; j < n; ++j) {
                fe_to_bytes_be(z[j], P, eb);
                sp.update(eb, 32);
            }
            fe_to_bytes_be(value, P, eb);
            sp.update(eb, 32);
        } else {
            memcpy(at, root, 32);
            sp.update(at, 32);
            at += 32;
        }
        for (int t = 0; t < 3; ++t) fe_to_bytes_be(hr[t], P, at + 32 * t);
        sp.update(at, 96);
        at += 96;
        betas[r] = squeeze_field_element(sp, P);
        scale = fe_mul(scale, ml_eq1(betas[r], z[r], P), P);
    }
    // layer R and the final polynomial: inverse transform over its coset, first 2^f coefficients
    const uint32_t nR = f + b;
    const uint64_t n_final = 1ull << f;
    ZKCHK(mle_alloc(c, nR, layers[R].put()));
    layer_at[R] = layers[R]->d;
    ZKCHK(fri_fold2(c, plan.get(), layer_at[R - 1], nR + 1, R - 1, s_inv, betas[R - 1], layers[R]->d));
    s_inv = fe_sqr(s_inv, P);
    ZKCHK(mle_alloc(c, nR, coeffs.put()));
    ZKCHK(zk_ntt(c, layers[R].get(), 1, coeffs.get()));
    {
        uint64_t base[4], one[4];
        fe_to_u64limbs(s_inv, base);
        fe_to_u64limbs(fe_one(P), one);
        ZKCHK(zk_mle_mul_powers(c, coeffs.get(), base, one));
    }
    try {
        staged.resize(4 * n_final);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    HIPCHK(hipMemcpyAsync(staged.data(), coeffs->d, (size_t)n_final * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint64_t j = 0; j < n_final; ++j) fe_to_bytes_be(fe_from_u64limbs(staged.data() + 4 * j), P, at + 32 * j);
    sp.update(at, (size_t)n_final * 32);
    at += n_final * 32;
    // the queries: every layer opened for all of them with one gather launch each, one download
    for (uint32_t q = 0; q < Q; ++q) idx[q] = fri_query_index(sp, n0 - 1);
    uint64_t per_query = 0;
    for (uint32_t r = 0; r < R; ++r) per_query += 2 + n0 - 1 - r;
    try {
        staged.resize(4 * Q * per_query);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    ZKCHK(d_idx.alloc(c, ml_scratch_bytes((size_t)Q * 8)));
    ZKCHK(d_stage.alloc(c, ml_scratch_bytes((size_t)Q * per_query * 32)));
    HIPCHK(hipMemcpyAsync(d_idx.p, idx.data(), (size_t)Q * 8, hipMemcpyHostToDevice, c->stream));
    uint64_t off = 0;   // in elements of the staging block: layer r's rows, then its paths
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t m = n0 - 1 - r;
        uint64_t *rows = d_stage.as() + 4 * off, *paths = rows + 4 * (2ull * Q);
        ZKCHK(fri_gather(c, layer_at[r], tree_at[r], m, 2, d_idx.as(), Q, rows, paths));
        off += (uint64_t)Q * (2 + m);
    }
    HIPCHK(hipMemcpyAsync(staged.data(), d_stage.p, (size_t)Q * per_query * 32, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    for (uint32_t q = 0; q < Q; ++q) {
        off = 0;
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t m = n0 - 1 - r;
            const uint64_t *rows = staged.data() + 4 * (off + 2ull * q), *paths = staged.data() + 4 * (off + 2ull * Q + (uint64_t)q * m);
            for (uint32_t j = 0; j < 2; ++j, at += 32) fe_to_bytes_be(fe_from_u64limbs(rows + 4 * j), P, at);
            memcpy(at, paths, (size_t)m * 32);
            at += (size_t)m * 32;
            off += (uint64_t)Q * (2 + m);
        }
    }
    fe_to_u64limbs(value, out_value);
    memcpy(out_proof, proof.data(), proof.size());
    return ZK_OK;
}

// ---- the verifier: host only, no context -----------------------------------------------------------------------------------------------
extern "C" int32_t zk_mlpcs_verify_host(int32_t field, uint32_t n_vars, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries,
                                        const uint64_t shift[4], const uint8_t seed[32], const uint8_t root[32], const uint64_t *point,
                                        const uint64_t value[4], const uint8_t *proof, uint64_t proof_len, int32_t *out_ok) {
    if (!shift || !seed || !root || !point || !value || !proof || !out_ok) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    const uint32_t n = n_vars, b = log_blowup, f = log_final, Q = n_queries;
    uint64_t want_len = 0;
    ZKCHK(zk_mlpcs_proof_bytes(n, b, f, Q, &want_len));
    Fe s0, v;
    if (!fri_elem(shift, P, &s0) || fe_is_zero(s0) || !fri_elem(value, P, &v) || proof_len != want_len) return ZK_ERR_BAD_ARG;
    const uint32_t n0 = n + b, R = n - f;
    std::vector<Fe> z, beta, s_inv, w_inv, final_co;
    std::vector<const uint8_t *> roots;
    try {
        z.resize(n);
        beta.resize(R);
        s_inv.resize(R);
        w_inv.resize(R);
        roots.resize(R);
        final_co.resize((size_t)1 << f);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (uint32_t j = 0; j < n; ++j)
        if (!fri_elem(point + 4 * j, P, &z[j])) return ZK_ERR_BAD_ARG;
    if (n0 > fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    *out_ok = 0;
    Sponge sp;
    sp.init();
    sp.update(seed, 32);
    {
        const uint64_t pv[5] = {(uint64_t)field, n, b, f, Q};
        uint8_t be[40], eb[32];
        for (int i = 0; i < 5; ++i)
            for (int k = 0; k < 8; ++k) be[8 * i + k] = (uint8_t)(pv[i] >> (8 * (7 - k)));
        sp.update(be, 40);
        fe_to_bytes_be(s0, P, eb);
        sp.update(eb, 32);
        sp.update(root, 32);
        for (uint32_t j = 0; j < n; ++j) {
            fe_to_bytes_be(z[j], P, eb);
            sp.update(eb, 32);
        }
        fe_to_bytes_be(v, P, eb);
        sp.update(eb, 32);
    }
    const Fe half = fe_inverse(fe_from_u32(2, P), P);
    const uint8_t *at = proof;
    Fe claim = v, scale = fe_one(P), s = s0;
    roots[0] = root;
    for (uint32_t r = 0; r < R; ++r) {
        if (r) {
            roots[r] = at;
            sp.update(at, 32);
            at += 32;
        }
        Fe hr[3];
        for (int t = 0; t < 3; ++t)
            if (!fri_from_be32(at + 32 * t, P, &hr[t])) return ZK_OK;   // not canonical: a verdict, not an error
        if (!fe_eq(fe_add(hr[0], hr[1], P), claim)) return ZK_OK;
        sp.update(at, 96);
        at += 96;
        beta[r] = squeeze_field_element(sp, P);
        claim = ml_quadratic_at(hr, beta[r], half, P);
        scale = fe_mul(scale, ml_eq1(beta[r], z[r], P), P);
        Fe w;
        field_root_of_unity(*fi, n0 - r, w);
        s_inv[r] = fe_inverse(s, P);
        w_inv[r] = fe_inverse(w, P);
        s = fe_sqr(s, P);
    }
    for (size_t j = 0; j < final_co.size(); ++j)
        if (!fri_from_be32(at + 32 * j, P, &final_co[j])) return ZK_OK;
    sp.update(at, 32 * final_co.size());
    at += 32 * final_co.size();
    // claim_R = scale * sum_key final[key] prod_{v in key} z_{R+v}: the coefficient form of T_R at the rest of the point
    Fe t_r = fe_zero();
    for (size_t key = 0; key < final_co.size(); ++key) {
        Fe term = final_co[key];
        for (uint32_t vb = 0; vb < f; ++vb)
            if (key >> vb & 1) term = fe_mul(term, z[R + vb], P);
        t_r = fe_add(t_r, term, P);
    }
    if (!fe_eq(claim, fe_mul(scale, t_r, P))) return ZK_OK;
    Fe w_last;   // layer R: 2^(f+b) points over the coset of s (= s_R by now)
    field_root_of_unity(*fi, f + b, w_last);
    for (uint32_t q = 0; q < Q; ++q) {
        uint64_t idx = fri_query_index(sp, n0 - 1);
        Fe y = fe_zero();
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t m = n0 - 1 - r;
            const uint64_t rho = idx & ((1ull << m) - 1);
            Fe row[2];
            uint64_t limbs[8];
            for (uint32_t j = 0; j < 2; ++j) {
                if (!fri_from_be32(at + 32 * j, P, &row[j])) return ZK_OK;
                fe_to_u64limbs(row[j], limbs + 4 * j);
            }
            at += 64;
            int32_t ok = 0;
            ZKCHK(zk_merkle_verify_host(field, roots[r], m, 2, rho, limbs, at, &ok));
            at += 32 * (size_t)m;
            if (!ok) return ZK_OK;
            if (r > 0 && !fe_eq(row[idx >> m], y)) return ZK_OK;
            const Fe x_inv = fe_mul(s_inv[r], fe_pow_u64(w_inv[r], rho, P), P);
            y = fri_fold_row(row, 1, x_inv, beta[r], half, *fi);
            idx = rho;
        }
        const Fe x = fe_mul(s, fe_pow_u64(w_last, idx, P), P);
        Fe g = fe_zero();
        for (size_t j = final_co.size(); j-- > 0;) g = fe_add(fe_mul(g, x, P), final_co[j], P);
        if (!fe_eq(g, y)) return ZK_OK;
    }
    *out_ok = 1;
    return ZK_OK;
}

// ---- the two sums of one round, public in its own right ----------------------------------------------------------------------------------
extern "C" int32_t zk_mle_eq_sums(zk_ctx *c, const zk_mle *t, const uint64_t *tail, uint64_t out[8]) {
    if (!c || !t || !out || (!tail && t->n_vars > 1)) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (t->n_vars < 1 || t->n_vars > kMaxVars) return ZK_ERR_BAD_ARG;
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)t->n_vars;
    uint64_t point[4 * (kMaxVars + 1)] = {};   // z_0 = 0 never enters a sum
    for (uint32_t j = 0; j + 1 < n; ++j) {
        Fe e;
        if (!fri_elem(tail + 4 * j, P, &e)) return ZK_ERR_BAD_ARG;
        memcpy(point + 4 * (j + 1), tail + 4 * j, 32);
    }
    ZKCHK(use_device(c));
    RoundSide side;
    PoolBlock d_out;
    DrainOnExit drain(c);
    ZKCHK(d_out.alloc(c, 64));
    ZKCHK(side.init(c, t->d, n, point, true));
    ZKCHK(side.round(0, fe_zero(), d_out.as()));
    HIPCHK(hipMemcpyAsync(c->h_pinned, d_out.p, 64, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    memcpy(out, c->h_pinned, 64);
    return ZK_OK;
}

// device time of the whole sumcheck side of `reps` openings of the table (all n_vars rounds: the eq factors, round 0's sums, then per
// round the fold joined to the sums; fixed point and challenges, no transcript and no host wait between rounds) between two HIP events
// after as many untimed ones: path 0 = as the switch decides, 1 = the fused round kernel, 2 = the eq table with the two-table round sums
// and two folds per round.  The table is left intact.
extern "C" int32_t zk_bench_mlpcs_round(zk_ctx *c, const zk_mle *t, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !t || !out_ms || reps < 1 || path < 0 || path > 2) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (t->n_vars < 1 || t->n_vars > kMaxVars) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)t->n_vars;
    const bool fused = path == kMlPathDefault ? mlpcs_fused_round() : path == kMlPathFused;
    uint64_t point[4 * kMaxVars];
    Fe e = c->fi->two_adic_root;   // any elements
    for (uint32_t j = 0; j < n; ++j, e = fe_add(fe_sqr(e, P), fe_one(P), P)) fe_to_u64limbs(e, point + 4 * j);
    const Fe beta = fe_from_u32(c->fi->generator, P);
    PoolBlock d_out;
    DrainOnExit drain(c);
    ZKCHK(d_out.alloc(c, 128));
    auto once = [&]() -> int32_t {
        RoundSide side;   // its blocks go back stream-ordered and come out of the pool again on the next call
        ZKCHK(side.init(c, t->d, n, point, fused));
        for (uint32_t r = 0; r < n; ++r) ZKCHK(side.round(r, beta, d_out.as()));
        return ZK_OK;
    };
    ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
    drain.armed = false;   // the span has waited for ev1
    return ZK_OK;
}
