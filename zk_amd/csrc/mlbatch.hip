// mlbatch.hip -- host side of the batch multilinear commitment (kernels in mlbatch_kernels.cuh; no reference item, definition:
// tests/mlbatch_ref.py): k tables of one size under one Merkle tree, opened at m points by ONE BaseFold opening
// (mlpcs.hip) of T_0 = sum_c lambda^c t_c against E_0 = sum_j gamma^j eq(., z_j).  The handle keeps copies of the tables and the k layers
// F_0^c in one contiguous block each (codeword c at c 2^(n+b): the tree's 2k columns are consecutive blocks of M_0 elements, so fri.hip's
// gather serves layer 0 with width 2k).  The opening: the m x k values from the sum-only form of the round kernel (one wait, with the
// root); round 0's sums follow from those on the host; T_0 by the linear-combination kernel; F_1 by the combine-and-fold kernel (or,
// ZK_MLBATCH_FUSE_FOLD=0, the linear combination into a scratch layer and FRI's fold: the same bytes); from there mlpcs.hip's rounds with
// the round kernel for several points (the folding pass takes the first kMlPointsPerPass points, sum-only passes over the just-written T_r
// the rest).  The shapes, the proof's length and the sumcheck's host arithmetic are ml_host.hpp's, shared with mlpcs.hip.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "ml_host.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "mlbatch_kernels.cuh"

// ZK_MLBATCH_FUSE_FOLD: 1 = k_ml_combine_fold, 0 = k_ml_lincomb into a scratch layer, then fri_fold2 (DESIGN.md section 19 has the
// measurement behind the default)
constexpr uint32_t kMlBatchFuseDefault = 1;
static bool mlbatch_fuse_fold() {
    static const bool fused = env_u64("ZK_MLBATCH_FUSE_FOLD", kMlBatchFuseDefault, 0, 1) != 0;
    return fused;
}
constexpr uint32_t kMlBatchMaxTables = 256, kMlBatchMaxPoints = 16;
enum { kMbPathOpen = 0, kMbPathFused = 1, kMbPathUnfused = 2, kMbPathManyRound = 3, kMbPathSingleRounds = 4 };

struct zk_mlbatch {
    zk_ctx *ctx;
    uint32_t n, b, k;
    Fe shift;
    PoolBlock tables;   // the k tables, table c at c 2^n: read only
    PoolBlock lde;      // the k layers F_0^c, codeword c at c 2^(n+b); column j of the tree is its j-th block of M_0 elements
    PoolBlock tree;     // every level over M_0 = 2^(n+b-1) rows of 2k columns
    PoolBlock ptrs;     // device pointer tables for k_ml_lincomb: k table pointers, then k codeword pointers
    const uint64_t *table(uint32_t c) const { return tables.as() + 4 * ((uint64_t)c << n); }
    const uint64_t *const *table_ptrs() const { return ptrs.as<const uint64_t *>(); }
    const uint64_t *const *codeword_ptrs() const { return ptrs.as<const uint64_t *>() + k; }
};
static void mlbatch_release(zk_mlbatch *h) { delete h; }   // the blocks go back to the pool with their owner
using MlBatchHolder = Scoped<zk_mlbatch, mlbatch_release>;
using FoldPlanHolder = Scoped<FriFoldPlan, fri_fold_plan_release>;

// ptrs[c] = tables + c * t_words (c < k), ptrs[k + c] = lde + c * l_words: the handle's pointer tables without a host copy
static __global__ __launch_bounds__(kBlock) void k_mlbatch_ptrs(const uint64_t *tables, uint64_t t_words, const uint64_t *lde, uint64_t l_words, uint32_t k,
                                                                const uint64_t **ptrs) {
    const uint32_t t = threadIdx.x;
    if (t < k) ptrs[t] = tables + (uint64_t)t * t_words;
    if (t < k) ptrs[k + t] = lde + (uint64_t)t * l_words;
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
static int32_t lincomb_launch(zk_ctx *c, const uint64_t *const *d_srcs, uint32_t k, const Mul29 *d_coef, uint64_t *out, uint64_t n_elems) {
    if (n_elems >= 64) {
        const uint64_t want = (n_elems + (uint64_t)kBlock * kLincombPerThread - 1) / ((uint64_t)kBlock * kLincombPerThread);
        k_ml_lincomb<true><<<(uint32_t)(want < kLincombMaxGrid ? want : kLincombMaxGrid), kBlock, 0, c->stream>>>(d_srcs, k, d_coef, out, n_elems, c->fi->P);
    } else {
        k_ml_lincomb<false><<<1, kBlock, 0, c->stream>>>(d_srcs, k, d_coef, out, n_elems, c->fi->P);
    }
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// F_1 (2^(n0-1) points) from the k codewords of 2^n0 points at base, stride apart, at beta over the coset of 1 / s_inv
static int32_t combine_fold_launch(zk_ctx *c, const FriFoldPlan *pl, const uint64_t *base, uint32_t n0, uint32_t k, const Mul29 *d_coef, const Fe &s_inv,
                                   const Fe &beta, uint64_t *out) {
    const FieldParams &P = c->fi->P;
    FriTable tw = {};
    fri_fold_plan_table(pl, &tw.lo, &tw.hi, &tw.lo_bits, &tw.hi_bits);
    tw.stride_log = 0;
    FriConsts kc = {};
    kc.c = mul29_prepare(fe_mul(beta, s_inv, P), P);
    const uint64_t M = 1ull << (n0 - 1), stride_words = 4ull << n0;
    if (M >= 64) {   // one 64-element run per wave, as fri.hip launches its fold
        uint64_t g = M / kBlock;
        if (g > 2 * kMaxGridStream) g = 2 * kMaxGridStream;
        k_ml_combine_fold<true><<<(uint32_t)(g ? g : 1), kBlock, 0, c->stream>>>(base, stride_words, k, d_coef, out, M, tw, kc, P);
    } else {
        k_ml_combine_fold<false><<<1, kBlock, 0, c->stream>>>(base, stride_words, k, d_coef, out, M, tw, kc, P);
    }
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// ---- the sumcheck side for several points: every point's Hi / Lo tables, passes of up to kMlPointsPerPass points ---------------------------
struct ManySide {
    zk_ctx *c = nullptr;
    uint32_t n = 0, np = 0, lo_max = 0, hi_max = 0;
    uint64_t hi_stride = 0, lo_stride = 0;   // words between two points' tables
    PoolBlock d_vars, hi, lo;
    // h_tails: np x (n - 1) elements in PINNED memory that stays untouched until the stream has passed the copy.  Enqueues only.
    int32_t init(zk_ctx *cc, uint32_t n_vars, const uint64_t *h_tails, uint32_t n_points) {
        c = cc, n = n_vars, np = n_points;
        const uint32_t nvars = n - 1;
        lo_max = nvars < kMlLoBits ? nvars : kMlLoBits;
        hi_max = nvars - lo_max;
        hi_stride = 8ull << hi_max, lo_stride = 8ull << lo_max;   // 2 << max elements of 4 words
        ZKCHK(d_vars.alloc(c, ml_scratch_bytes((size_t)np * nvars * 32)));
        ZKCHK(hi.alloc(c, (size_t)np * hi_stride * 8));
        ZKCHK(lo.alloc(c, (size_t)np * lo_stride * 8));
        if (nvars) HIPCHK(hipMemcpyAsync(d_vars.p, h_tails, (size_t)np * nvars * 32, hipMemcpyHostToDevice, c->stream));
        for (uint32_t j = 0; j < np; ++j) {
            k_ml_eq_tables<<<grid_for((2ull << hi_max) + (2ull << lo_max)), kBlock, 0, c->stream>>>(d_vars.as() + 4ull * j * nvars, nvars, lo_max, hi.as() + j * hi_stride,
                                                                                                   lo.as() + j * lo_stride, c->fi->P);
            HIPCHK(hipGetLastError());
        }
        return ZK_OK;
    }
    // one pass at the points j0 .. j0 + cnt (cnt <= kMlPointsPerPass) of the table of n_t variables whose tails are the LAST n_t - 1
    // variables of the points': fold (src = the table of n_t + 1 variables, folded at beta into dst and summed on the way) or sum-only
    // (src = the table itself) -> 2 cnt elements at d_out.  Enqueues only.
    int32_t pass(uint32_t n_t, const uint64_t *src, uint64_t *dst, bool fold, const Fe &beta, uint32_t j0, uint32_t cnt, uint64_t *d_out) {
        const FieldParams &P = c->fi->P;
        const uint32_t m = n_t - 1, L = m < kMlLoBits ? m : kMlLoBits;
        const uint64_t *hi_r = hi.as() + j0 * hi_stride + 4 * (1ull << (m - L)), *lo_r = lo.as() + j0 * lo_stride + 4 * (1ull << L);
        const Mul29 b29 = mul29_prepare(beta, P);
        const bool run = m >= kMlRunMinBits;
        uint32_t g = 1, S = 0;
        if (run) {   // mlpcs.hip's launch shape: a run per wave, as long as the Lo table allows where that still leaves 2^kMlRunsTargetLog runs
            const uint32_t fit = m > kMlRunsTargetLog + kMlRunMinBits ? m - kMlRunsTargetLog : kMlRunMinBits;
            S = fit < L ? fit : L;
            const uint64_t n_runs = 1ull << (m - S), want = (n_runs + kBlock / 64 - 1) / (kBlock / 64);
            g = (uint32_t)(want < kMaxGrid ? want : kMaxGrid);
        }
#define ZK_MANY_LAUNCH(NP, FOLD, RUN) \
    k_ml_round_many<NP, FOLD, RUN><<<g, kBlock, 0, c->stream>>>(src, dst, m, S, hi_r, hi_stride, lo_r, lo_stride, b29, c->d_partials, P)
#define ZK_MANY_SHAPE(NP)                         \
    do {                                          \
        if (fold && run) ZK_MANY_LAUNCH(NP, true, true);        \
        else if (fold) ZK_MANY_LAUNCH(NP, true, false);         \
        else if (run) ZK_MANY_LAUNCH(NP, false, true);          \
        else ZK_MANY_LAUNCH(NP, false, false);                  \
    } while (0)
        static_assert(kMlPointsPerPass == 4, "the dispatch below names every pass size");
        switch (cnt) {
        case 1: ZK_MANY_SHAPE(1); break;
        case 2: ZK_MANY_SHAPE(2); break;
        case 3: ZK_MANY_SHAPE(3); break;
        case 4: ZK_MANY_SHAPE(4); break;
        default: return ZK_ERR_BAD_ARG;
        }
#undef ZK_MANY_SHAPE
#undef ZK_MANY_LAUNCH
        HIPCHK(hipGetLastError());
        return launch_reduce_tail(c, g, 2 * cnt, d_out);
    }
    // the sums of the table of n_t variables at ALL points -> 2 np elements at d_out; fold: the first pass folds src into dst, the others
    // read dst; else every pass reads src
    int32_t all(uint32_t n_t, const uint64_t *src, uint64_t *dst, bool fold, const Fe &beta, uint64_t *d_out, uint32_t per_pass = kMlPointsPerPass) {
        for (uint32_t j0 = 0; j0 < np; j0 += per_pass) {
            const uint32_t cnt = np - j0 < per_pass ? np - j0 : per_pass;
            ZKCHK(pass(n_t, fold && j0 ? dst : src, dst, fold && j0 == 0, beta, j0, cnt, d_out + 8ull * j0));
        }
        return ZK_OK;
    }
};

// ---- the commitment ------------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_mlbatch_commit(zk_ctx *c, const zk_mle *const *tables, uint32_t k, uint32_t log_blowup, const uint64_t shift[4], zk_mlbatch **out) {
    if (!c || !tables || !shift || !out || k < 1 || k > kMlBatchMaxTables) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (!tables[j]) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (tables[j]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)tables[0]->n_vars, b = log_blowup;
    Fe s;
    if (tables[0]->n_vars < 1 || tables[0]->n_vars > kMaxVars || b < 1 || b > kMlMaxBlowupLog || !fri_elem(shift, P, &s) || fe_is_zero(s)) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 1; j < k; ++j)
        if (tables[j]->n_vars != tables[0]->n_vars) return ZK_ERR_BAD_ARG;
    const uint32_t n0 = n + b, m = n0 - 1;
    if (n0 > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    if (n0 > kMaxVars) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    MlBatchHolder h(new (std::nothrow) zk_mlbatch());
    if (!h.get()) return ZK_ERR_ALLOC;
    h->ctx = c, h->n = n, h->b = b, h->k = k, h->shift = s;
    std::vector<const uint64_t *> cols;
    try {
        cols.resize(2 * (size_t)k);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    PoolBlock coeffs;
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the blocks go back
    ZKCHK(h->tables.alloc(c, (size_t)k * mle_block_bytes(n)));
    ZKCHK(h->lde.alloc(c, (size_t)k * mle_block_bytes(n0)));
    ZKCHK(h->tree.alloc(c, (size_t)64 << m));
    ZKCHK(h->ptrs.alloc(c, ml_scratch_bytes((size_t)2 * k * sizeof(uint64_t *))));
    ZKCHK(coeffs.alloc(c, mle_block_bytes(n)));
    for (uint32_t j = 0; j < k; ++j) {
        uint64_t *cw = h->lde.as() + 4 * ((uint64_t)j << n0);
        HIPCHK(hipMemcpyAsync(const_cast<uint64_t *>(h->table(j)), tables[j]->d, mle_block_bytes(n), hipMemcpyDeviceToDevice, c->stream));
        ZKCHK(cmle_interpolate_into(c, tables[j], coeffs.as()));   // key bit v <-> variable v: coefficient j of the univariate polynomial
        const zk_upoly poly = {c, 1ull << n, coeffs.as()};
        zk_mle layer0 = {c, n0, cw};
        ZKCHK(fri_lde_into(c, &poly, n0, shift, &layer0));
        cols[2 * j] = cw, cols[2 * j + 1] = cw + 4 * (1ull << m);
    }
    ZKCHK(merkle_build_raw(c, cols.data(), 2 * k, m, h->tree.as()));
    k_mlbatch_ptrs<<<1, kBlock, 0, c->stream>>>(h->tables.as(), 4ull << n, h->lde.as(), 4ull << n0, k, h->ptrs.as<const uint64_t *>());
    HIPCHK(hipGetLastError());
    drain.armed = false;   // enqueued: the coefficients go back stream-ordered
    *out = h.release();
    return ZK_OK;
}
extern "C" int32_t zk_mlbatch_free(zk_mlbatch *h) {
    mlbatch_release(h);   // back to its context's pool; reuse is stream-ordered
    return ZK_OK;
}
extern "C" int32_t zk_mlbatch_n_vars(const zk_mlbatch *h, uint32_t *out) {
    if (!h || !out) return ZK_ERR_BAD_ARG;
    *out = h->n;
    return ZK_OK;
}
extern "C" int32_t zk_mlbatch_n_tables(const zk_mlbatch *h, uint32_t *out) {
    if (!h || !out) return ZK_ERR_BAD_ARG;
    *out = h->k;
    return ZK_OK;
}
extern "C" int32_t zk_mlbatch_root(zk_ctx *c, const zk_mlbatch *h, uint8_t out[32]) {
    if (!c || !h || !out) return ZK_ERR_BAD_ARG;
    if (h->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    const uint32_t m = h->n + h->b - 1;
    HIPCHK(hipMemcpyAsync(out, h->tree.as() + 4 * ((2ull << m) - 2), 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
static bool mlbatch_shape(uint32_t n, uint32_t k, uint32_t np, uint32_t b, uint32_t f, uint32_t q) {
    return ml_open_shape(n, b, f, q) && k >= 1 && k <= kMlBatchMaxTables && np >= 1 && np <= kMlBatchMaxPoints;
}
extern "C" int32_t zk_mlbatch_proof_bytes(uint32_t n_vars, uint32_t k, uint32_t n_points, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries,
                                          uint64_t *out) {
    if (!out) return ZK_ERR_BAD_ARG;
    if (!mlbatch_shape(n_vars, k, n_points, log_blowup, log_final, n_queries)) return ZK_ERR_BAD_ARG;
    *out = ml_proof_bytes(n_vars, log_blowup, log_final, n_queries, 2 * k);
    return ZK_OK;
}

// the transcript's head, shared by the prover and the verifier: seed | be64 x 7 | be32(s) | root | the points | the values -> lambda, gamma
static void mlbatch_start(Sponge &sp, int32_t field, uint32_t n, uint32_t b, uint32_t f, uint32_t Q, uint32_t k, uint32_t np, const Fe &shift,
                          const uint8_t seed[32], const uint8_t root[32], const std::vector<Fe> &z, const std::vector<Fe> &v, const FieldParams &P, Fe *lambda,
                          Fe *gamma) {
    sp.init();
    sp.update(seed, 32);
    const uint64_t pv[7] = {(uint64_t)field, n, b, f, Q, k, np};
    uint8_t be[56], eb[32];
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 8; ++j) be[8 * i + j] = (uint8_t)(pv[i] >> (8 * (7 - j)));
    sp.update(be, 56);
    fe_to_bytes_be(shift, P, eb);
    sp.update(eb, 32);
    sp.update(root, 32);
    for (const Fe &e : z) {
        fe_to_bytes_be(e, P, eb);
        sp.update(eb, 32);
    }
    for (const Fe &e : v) {
        fe_to_bytes_be(e, P, eb);
        sp.update(eb, 32);
    }
    *lambda = squeeze_field_element(sp, P);
    *gamma = squeeze_field_element(sp, P);
}
static void fe_powers(const Fe &x, std::vector<Fe> &out, const FieldParams &P) {
    Fe cur = fe_one(P);
    for (Fe &o : out) {
        o = cur;
        cur = fe_mul(cur, x, P);
    }
}

// ---- the opening ---------------------------------------------------------------------------------------------------------------------
// What one opening keeps on the device between its waits; the measurement hook drives the same steps with fixed challenges.
struct OpenState {
    zk_ctx *c;
    const zk_mlbatch *h;
    uint32_t n, b, k, np, n0, R;
    bool fuse;
    ManySide side;
    FoldPlanHolder plan;
    PoolBlock d_vals, d_coef, d_dl, t0, tbuf[2], scratch0;
    std::vector<MleHolder> layers;   // layers[r], r >= 1 (layer 0 is virtual: the commitment's codewords)
    std::vector<PoolBlock> trees;    // trees[r], r >= 1
    Fe s_inv;
    OpenState(zk_ctx *cc, const zk_mlbatch *hh, uint32_t n_points, uint32_t f, bool fuse_fold)
        : c(cc), h(hh), n(hh->n), b(hh->b), k(hh->k), np(n_points), n0(hh->n + hh->b), R(hh->n - f), fuse(fuse_fold) {}
    // h_tails: pinned, np x (n - 1) elements
    int32_t init(const uint64_t *h_tails) {
        try {
            layers.resize(R + 1);
            trees.resize(R);
        } catch (...) {
            return ZK_ERR_ALLOC;
        }
        ZKCHK(side.init(c, n, h_tails, np));
        ZKCHK(fri_fold_plan(c, n0, plan.put()));
        ZKCHK(d_vals.alloc(c, ml_scratch_bytes(32 + (size_t)k * np * 64)));   // root | [c][j][X]
        ZKCHK(d_coef.alloc(c, ml_scratch_bytes((size_t)k * sizeof(Mul29))));
        ZKCHK(d_dl.alloc(c, ml_scratch_bytes(32 + (size_t)np * 64)));         // root_r | the round's sums [j][X]
        if (R >= 2) {
            ZKCHK(t0.alloc(c, mle_block_bytes(n)));
            for (uint32_t j = 0; j < 2 && j + 2 <= n; ++j) ZKCHK(tbuf[j].alloc(c, mle_block_bytes(n - 1 - j)));
        }
        if (!fuse) ZKCHK(scratch0.alloc(c, mle_block_bytes(n0)));
        s_inv = fe_inverse(h->shift, c->fi->P);
        return ZK_OK;
    }
    // the sums of every table at every point and the root -> d_vals
    int32_t values() {
        for (uint32_t j = 0; j < k; ++j) ZKCHK(side.all(n, h->table(j), nullptr, false, fe_zero(), d_vals.as() + 4 + 8ull * j * np));
        HIPCHK(hipMemcpyAsync(d_vals.p, h->tree.as() + 4 * ((2ull << (n0 - 1)) - 2), 32, hipMemcpyDeviceToDevice, c->stream));
        return ZK_OK;
    }
    // h_coef: pinned, the k prepared powers of lambda; T_0 when a later round needs it
    int32_t combine(const Mul29 *h_coef) {
        HIPCHK(hipMemcpyAsync(d_coef.p, h_coef, (size_t)k * sizeof(Mul29), hipMemcpyHostToDevice, c->stream));
        if (R >= 2) ZKCHK(lincomb_launch(c, h->table_ptrs(), k, d_coef.as<Mul29>(), t0.as(), 1ull << n));
        return ZK_OK;
    }
    const uint64_t *t_at(uint32_t r) const { return r == 0 ? t0.as() : tbuf[(r - 1) & 1].as(); }
    // layer r (1 <= r <= R) from layer r - 1 at beta_{r-1}; r < R: its tree as well
    int32_t fold_to(uint32_t r, const Fe &beta) {
        const FieldParams &P = c->fi->P;
        const uint32_t nr = n0 - r, m = nr - 1;
        ZKCHK(mle_alloc(c, nr, layers[r].put()));
        if (r == 1 && fuse) ZKCHK(combine_fold_launch(c, plan.get(), h->lde.as(), n0, k, d_coef.as<Mul29>(), s_inv, beta, layers[1]->d));
        else {
            if (r == 1) ZKCHK(lincomb_launch(c, h->codeword_ptrs(), k, d_coef.as<Mul29>(), scratch0.as(), 1ull << n0));
            ZKCHK(fri_fold2(c, plan.get(), r == 1 ? scratch0.as() : layers[r - 1]->d, nr + 1, r - 1, s_inv, beta, layers[r]->d));
        }
        s_inv = fe_sqr(s_inv, P);
        if (r < R) {
            ZKCHK(trees[r].alloc(c, (size_t)64 << m));
            const uint64_t *cols[2] = {layers[r]->d, layers[r]->d + 4 * (1ull << m)};
            ZKCHK(merkle_build_raw(c, cols, 2, m, trees[r].as()));
        }
        return ZK_OK;
    }
    // round r >= 1: T_r = the fold of T_{r-1} at beta_{r-1}, its sums at every point and root_r -> d_dl
    int32_t round(uint32_t r, const Fe &beta) {
        ZKCHK(side.all(n - r, t_at(r - 1), tbuf[(r - 1) & 1].as(), true, beta, d_dl.as() + 4));
        HIPCHK(hipMemcpyAsync(d_dl.p, trees[r].as() + 4 * ((2ull << (n0 - r - 1)) - 2), 32, hipMemcpyDeviceToDevice, c->stream));
        return ZK_OK;
    }
    // the first 2^f coefficients of layer R over its coset -> coeffs (a table of f + b variables)
    int32_t final_poly(MleHolder &coeffs) {
        const FieldParams &P = c->fi->P;
        ZKCHK(mle_alloc(c, n0 - R, coeffs.put()));
        ZKCHK(zk_ntt(c, layers[R].get(), 1, coeffs.get()));
        uint64_t base[4], one[4];
        fe_to_u64limbs(s_inv, base);
        fe_to_u64limbs(fe_one(P), one);
        return zk_mle_mul_powers(c, coeffs.get(), base, one);
    }
};

extern "C" int32_t zk_mlbatch_open(zk_ctx *c, const zk_mlbatch *h, const uint64_t *points, uint32_t n_points, uint32_t log_final, uint32_t n_queries,
                                   const uint8_t seed[32], uint64_t *out_values, uint8_t *out_proof) {
    if (!c || !h || !points || !seed || !out_values || !out_proof) return ZK_ERR_BAD_ARG;
    if (h->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const FieldParams &P = c->fi->P;
    const uint32_t n = h->n, b = h->b, k = h->k, np = n_points, f = log_final, Q = n_queries, n0 = n + b;
    if (!mlbatch_shape(n, k, np, b, f, Q)) return ZK_ERR_BAD_ARG;
    const uint32_t R = n - f;
    std::vector<Fe> z, v, lp, gp, scale, betas;
    std::vector<uint64_t> idx, staged;
    std::vector<uint8_t> proof;
    try {
        z.resize((size_t)np * n);
        v.resize((size_t)np * k);
        lp.resize(k);
        gp.resize(np);
        scale.resize(np);
        betas.resize(R);
        idx.resize(Q);
        proof.resize(ml_proof_bytes(n, b, f, Q, 2 * k));
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (size_t j = 0; j < z.size(); ++j)
        if (!fri_elem(points + 4 * j, P, &z[j])) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    // pinned staging: the download of the root and the sums | the prepared coefficients | the points' tails
    const size_t dl_bytes = 32 + (size_t)k * np * 64, coef_at = (dl_bytes + 63) & ~(size_t)63, tails_at = (coef_at + (size_t)k * sizeof(Mul29) + 63) & ~(size_t)63;
    uint8_t *stage = nullptr;
    ZKCHK(results_staging(c, tails_at + (size_t)np * n * 32 + 64, &stage));
    uint64_t *h_tails = reinterpret_cast<uint64_t *>(stage + tails_at);
    for (uint32_t j = 0; j < np; ++j) memcpy(h_tails + 4ull * j * (n - 1), points + 4ull * (j * n + 1), (size_t)(n - 1) * 32);
    // owners first, the drain last: a call that leaves early waits for the stream before any block goes back
    OpenState st(c, h, np, f, mlbatch_fuse_fold());
    PoolBlock d_idx, d_stage;
    MleHolder coeffs;
    DrainOnExit drain(c);
    ZKCHK(st.init(h_tails));
    ZKCHK(st.values());
    HIPCHK(hipMemcpyAsync(stage, st.d_vals.p, dl_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the wait for the root and the values
    const uint64_t *h_sums = reinterpret_cast<const uint64_t *>(stage + 32);   // [c][j][X]
    uint8_t root[32];
    memcpy(root, stage, 32);
    const Fe one = fe_one(P);
    for (uint32_t j = 0; j < np; ++j)
        for (uint32_t t = 0; t < k; ++t) {   // v = (1 - z_0) S_0 + z_0 S_1
            const Fe s0 = fe_from_u64limbs(h_sums + 8ull * (t * np + j)), s1 = fe_from_u64limbs(h_sums + 8ull * (t * np + j) + 4), z0 = z[(size_t)j * n];
            v[(size_t)j * k + t] = fe_add(fe_mul(fe_sub(one, z0, P), s0, P), fe_mul(z0, s1, P), P);
        }
    Sponge sp;
    Fe lambda, gamma;
    mlbatch_start(sp, c->field, n, b, f, Q, k, np, h->shift, seed, root, z, v, P, &lambda, &gamma);
    fe_powers(lambda, lp, P);
    fe_powers(gamma, gp, P);
    uint8_t *at = proof.data();
    {   // round 0 on the host: the sums of T_0 are the lambda-combination of the tables' own
        Fe hr[3] = {fe_zero(), fe_zero(), fe_zero()};
        for (uint32_t j = 0; j < np; ++j) {
            Fe s0 = fe_zero(), s1 = fe_zero(), one_h[3];
            for (uint32_t t = 0; t < k; ++t) {
                s0 = fe_add(s0, fe_mul(lp[t], fe_from_u64limbs(h_sums + 8ull * (t * np + j)), P), P);
                s1 = fe_add(s1, fe_mul(lp[t], fe_from_u64limbs(h_sums + 8ull * (t * np + j) + 4), P), P);
            }
            scale[j] = gp[j];
            ml_round_poly(s0, s1, scale[j], z[(size_t)j * n], P, one_h);
            for (int t = 0; t < 3; ++t) hr[t] = fe_add(hr[t], one_h[t], P);
        }
        for (int t = 0; t < 3; ++t) fe_to_bytes_be(hr[t], P, at + 32 * t);
        sp.update(at, 96);
        at += 96;
        betas[0] = squeeze_field_element(sp, P);
        for (uint32_t j = 0; j < np; ++j) scale[j] = fe_mul(scale[j], ml_eq1(betas[0], z[(size_t)j * n], P), P);
    }
    Mul29 *h_coef = reinterpret_cast<Mul29 *>(stage + coef_at);
    for (uint32_t t = 0; t < k; ++t) h_coef[t] = mul29_prepare(lp[t], P);
    ZKCHK(st.combine(h_coef));
    for (uint32_t r = 1; r < R; ++r) {
        ZKCHK(st.fold_to(r, betas[r - 1]));
        ZKCHK(st.round(r, betas[r - 1]));
        HIPCHK(hipMemcpyAsync(c->h_pinned, st.d_dl.p, 32 + (size_t)np * 64, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));   // the round's one host wait
        memcpy(at, c->h_pinned, 32);
        sp.update(at, 32);
        at += 32;
        Fe hr[3] = {fe_zero(), fe_zero(), fe_zero()};
        for (uint32_t j = 0; j < np; ++j) {
            Fe one_h[3];
            ml_round_poly(fe_from_u64limbs(c->h_pinned + 4 + 8 * j), fe_from_u64limbs(c->h_pinned + 8 + 8 * j), scale[j], z[(size_t)j * n + r], P, one_h);
            for (int t = 0; t < 3; ++t) hr[t] = fe_add(hr[t], one_h[t], P);
        }
        for (int t = 0; t < 3; ++t) fe_to_bytes_be(hr[t], P, at + 32 * t);
        sp.update(at, 96);
        at += 96;
        betas[r] = squeeze_field_element(sp, P);
        for (uint32_t j = 0; j < np; ++j) scale[j] = fe_mul(scale[j], ml_eq1(betas[r], z[(size_t)j * n + r], P), P);
    }
    // layer R and the final polynomial: inverse transform over its coset, first 2^f coefficients
    const uint64_t n_final = 1ull << f;
    ZKCHK(st.fold_to(R, betas[R - 1]));
    ZKCHK(st.final_poly(coeffs));
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
    // the queries: every layer opened for all of them with one gather launch each (layer 0: the commitment's rows of 2k), one download
    for (uint32_t q = 0; q < Q; ++q) idx[q] = fri_query_index(sp, n0 - 1);
    const uint64_t per_query = ml_per_query(n, b, f, 2 * k);
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
        const uint32_t m = n0 - 1 - r, width = r ? 2 : 2 * k;
        uint64_t *rows = d_stage.as() + 4 * off, *paths = rows + 4 * ((uint64_t)width * Q);
        ZKCHK(fri_gather(c, r ? st.layers[r]->d : h->lde.as(), r ? st.trees[r].as() : h->tree.as(), m, width, d_idx.as(), Q, rows, paths));
        off += (uint64_t)Q * (width + m);
    }
    HIPCHK(hipMemcpyAsync(staged.data(), d_stage.p, (size_t)Q * per_query * 32, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    for (uint32_t q = 0; q < Q; ++q) {
        off = 0;
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t m = n0 - 1 - r, width = r ? 2 : 2 * k;
            const uint64_t *rows = staged.data() + 4 * (off + (uint64_t)width * q), *paths = staged.data() + 4 * (off + (uint64_t)width * Q + (uint64_t)q * m);
            for (uint32_t j = 0; j < width; ++j, at += 32) fe_to_bytes_be(fe_from_u64limbs(rows + 4 * j), P, at);
            memcpy(at, paths, (size_t)m * 32);
            at += (size_t)m * 32;
            off += (uint64_t)Q * (width + m);
        }
    }
    for (size_t j = 0; j < v.size(); ++j) fe_to_u64limbs(v[j], out_values + 4 * j);
    memcpy(out_proof, proof.data(), proof.size());
    return ZK_OK;
}

// ---- the verifier: host only, no context -----------------------------------------------------------------------------------------------
extern "C" int32_t zk_mlbatch_verify_host(int32_t field, uint32_t n_vars, uint32_t k, uint32_t n_points, uint32_t log_blowup, uint32_t log_final,
                                          uint32_t n_queries, const uint64_t shift[4], const uint8_t seed[32], const uint8_t root[32],
                                          const uint64_t *points, const uint64_t *values, const uint8_t *proof, uint64_t proof_len, int32_t *out_ok) {
    if (!shift || !seed || !root || !points || !values || !proof || !out_ok) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    const uint32_t n = n_vars, b = log_blowup, f = log_final, Q = n_queries, np = n_points;
    uint64_t want_len = 0;
    ZKCHK(zk_mlbatch_proof_bytes(n, k, np, b, f, Q, &want_len));
    Fe s0;
    if (!fri_elem(shift, P, &s0) || fe_is_zero(s0) || proof_len != want_len) return ZK_ERR_BAD_ARG;
    const uint32_t n0 = n + b, R = n - f;
    std::vector<Fe> z, v, lp, gp, beta, s_inv, w_inv, final_co, row;
    std::vector<uint64_t> limbs;
    std::vector<const uint8_t *> roots;
    try {
        z.resize((size_t)np * n);
        v.resize((size_t)np * k);
        lp.resize(k);
        gp.resize(np);
        beta.resize(R);
        s_inv.resize(R);
        w_inv.resize(R);
        roots.resize(R);
        final_co.resize((size_t)1 << f);
        row.resize(2 * (size_t)k);
        limbs.resize(8 * (size_t)k);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (size_t j = 0; j < z.size(); ++j)
        if (!fri_elem(points + 4 * j, P, &z[j])) return ZK_ERR_BAD_ARG;
    for (size_t j = 0; j < v.size(); ++j)
        if (!fri_elem(values + 4 * j, P, &v[j])) return ZK_ERR_BAD_ARG;
    if (n0 > fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    *out_ok = 0;
    Sponge sp;
    Fe lambda, gamma;
    mlbatch_start(sp, field, n, b, f, Q, k, np, s0, seed, root, z, v, P, &lambda, &gamma);
    fe_powers(lambda, lp, P);
    fe_powers(gamma, gp, P);
    Fe claim = fe_zero();
    for (uint32_t j = 0; j < np; ++j) {
        Fe acc = fe_zero();
        for (uint32_t t = 0; t < k; ++t) acc = fe_add(acc, fe_mul(lp[t], v[(size_t)j * k + t], P), P);
        claim = fe_add(claim, fe_mul(gp[j], acc, P), P);
    }
    const Fe half = fe_inverse(fe_from_u32(2, P), P);
    const uint8_t *at = proof;
    Fe s = s0;
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
    // claim_R = sum_j gamma^j prod_r eq1(beta_r, z_{j,r}) sum_key final[key] prod_{v in key} z_{j,R+v}
    Fe want = fe_zero();
    for (uint32_t j = 0; j < np; ++j) {
        const Fe *zj = z.data() + (size_t)j * n;
        Fe scale = gp[j], t_r = fe_zero();
        for (uint32_t r = 0; r < R; ++r) scale = fe_mul(scale, ml_eq1(beta[r], zj[r], P), P);
        for (size_t key = 0; key < final_co.size(); ++key) {
            Fe term = final_co[key];
            for (uint32_t vb = 0; vb < f; ++vb)
                if (key >> vb & 1) term = fe_mul(term, zj[R + vb], P);
            t_r = fe_add(t_r, term, P);
        }
        want = fe_add(want, fe_mul(scale, t_r, P), P);
    }
    if (!fe_eq(claim, want)) return ZK_OK;
    Fe w_last;   // layer R: 2^(f+b) points over the coset of s (= s_R by now)
    field_root_of_unity(*fi, f + b, w_last);
    for (uint32_t q = 0; q < Q; ++q) {
        uint64_t idx = fri_query_index(sp, n0 - 1);
        Fe y = fe_zero();
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t m = n0 - 1 - r, width = r ? 2 : 2 * k;
            const uint64_t rho = idx & ((1ull << m) - 1);
            for (uint32_t j = 0; j < width; ++j) {
                if (!fri_from_be32(at + 32 * j, P, &row[j])) return ZK_OK;
                fe_to_u64limbs(row[j], limbs.data() + 4 * j);
            }
            at += 32 * (size_t)width;
            int32_t ok = 0;
            ZKCHK(zk_merkle_verify_host(field, roots[r], m, width, rho, limbs.data(), at, &ok));
            at += 32 * (size_t)m;
            if (!ok) return ZK_OK;
            Fe pair[2];
            if (r == 0) {   // the pair of the virtual layer 0
                pair[0] = pair[1] = fe_zero();
                for (uint32_t t = 0; t < k; ++t) {
                    pair[0] = fe_add(pair[0], fe_mul(lp[t], row[2 * t], P), P);
                    pair[1] = fe_add(pair[1], fe_mul(lp[t], row[2 * t + 1], P), P);
                }
            } else {
                if (!fe_eq(row[idx >> m], y)) return ZK_OK;
                pair[0] = row[0], pair[1] = row[1];
            }
            const Fe x_inv = fe_mul(s_inv[r], fe_pow_u64(w_inv[r], rho, P), P);
            y = fri_fold_row(pair, 1, x_inv, beta[r], half, *fi);
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

// ---- the two device pieces, public in their own right ------------------------------------------------------------------------------------
extern "C" int32_t zk_mle_lincomb(zk_ctx *c, const zk_mle *const *tables, uint32_t k, const uint64_t *coeffs, zk_mle *out) {
    if (!c || !tables || !coeffs || !out || k < 1 || k > kMlBatchMaxTables) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (!tables[j]) return ZK_ERR_BAD_ARG;
    if (out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    for (uint32_t j = 0; j < k; ++j)
        if (tables[j]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const FieldParams &P = c->fi->P;
    if (out->n_vars > kMaxVars) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (tables[j]->n_vars != out->n_vars || tables[j]->d == out->d) return ZK_ERR_BAD_ARG;
    uint8_t *stage = nullptr;
    const size_t coef_at = ((size_t)k * sizeof(uint64_t *) + 63) & ~(size_t)63, bytes = coef_at + (size_t)k * sizeof(Mul29);
    std::vector<Fe> cf;
    try {
        cf.resize(k);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (uint32_t j = 0; j < k; ++j)
        if (!fri_elem(coeffs + 4 * j, P, &cf[j])) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    ZKCHK(results_staging(c, bytes, &stage));
    PoolBlock d_args;
    DrainOnExit drain(c);
    ZKCHK(d_args.alloc(c, ml_scratch_bytes(bytes)));
    const uint64_t **h_ptrs = reinterpret_cast<const uint64_t **>(stage);
    Mul29 *h_coef = reinterpret_cast<Mul29 *>(stage + coef_at);
    for (uint32_t j = 0; j < k; ++j) h_ptrs[j] = tables[j]->d, h_coef[j] = mul29_prepare(cf[j], P);
    HIPCHK(hipMemcpyAsync(d_args.p, stage, bytes, hipMemcpyHostToDevice, c->stream));
    ZKCHK(lincomb_launch(c, d_args.as<const uint64_t *>(), k, reinterpret_cast<const Mul29 *>(d_args.as<uint8_t>() + coef_at), out->d, 1ull << out->n_vars));
    return drain.wait();   // the staging is free again
}
extern "C" int32_t zk_mle_eq_sums_many(zk_ctx *c, const zk_mle *t, const uint64_t *tails, uint32_t n_points, uint64_t *out) {
    if (!c || !t || !out || (!tails && t->n_vars > 1)) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (t->n_vars < 1 || t->n_vars > kMaxVars || n_points < 1 || n_points > kMlBatchMaxPoints) return ZK_ERR_BAD_ARG;
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)t->n_vars, np = n_points;
    const size_t tail_bytes = (size_t)np * (n - 1) * 32, dl_at = (tail_bytes + 63) & ~(size_t)63;
    for (size_t j = 0; j < (size_t)np * (n - 1); ++j) {
        Fe e;
        if (!fri_elem(tails + 4 * j, P, &e)) return ZK_ERR_BAD_ARG;
    }
    ZKCHK(use_device(c));
    uint8_t *stage = nullptr;
    ZKCHK(results_staging(c, dl_at + (size_t)np * 64, &stage));
    if (tail_bytes) memcpy(stage, tails, tail_bytes);
    ManySide side;
    PoolBlock d_out;
    DrainOnExit drain(c);
    ZKCHK(d_out.alloc(c, ml_scratch_bytes((size_t)np * 64)));
    ZKCHK(side.init(c, n, reinterpret_cast<const uint64_t *>(stage), np));
    ZKCHK(side.all(n, t->d, nullptr, false, fe_zero(), d_out.as()));
    HIPCHK(hipMemcpyAsync(stage + dl_at, d_out.p, (size_t)np * 64, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    memcpy(out, stage + dl_at, (size_t)np * 64);
    return ZK_OK;
}

// device time of `reps` runs between two HIP events after as many untimed ones (timing.hpp): see include/zk_amd.h for the paths.  Fixed
// points and challenges; nothing of the handle is written.
extern "C" int32_t zk_bench_mlbatch(zk_ctx *c, const zk_mlbatch *h, uint32_t n_points, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !h || !out_ms || reps < 1 || path < 0 || path > 4) return ZK_ERR_BAD_ARG;
    if (h->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (path == kMbPathOpen && (n_points < 1 || n_points > kMlBatchMaxPoints)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const FieldParams &P = c->fi->P;
    const uint32_t n = h->n, k = h->k, n0 = n + h->b;
    const uint32_t np = path == kMbPathOpen ? n_points : kMlPointsPerPass;
    const Fe beta = fe_from_u32(c->fi->generator, P);
    uint8_t *stage = nullptr;
    const size_t coef_at = ((size_t)np * n * 32 + 63) & ~(size_t)63;
    ZKCHK(results_staging(c, coef_at + (size_t)k * sizeof(Mul29), &stage));
    uint64_t *h_tails = reinterpret_cast<uint64_t *>(stage);
    Mul29 *h_coef = reinterpret_cast<Mul29 *>(stage + coef_at);
    Fe e = c->fi->two_adic_root;   // any elements
    for (size_t j = 0; j < (size_t)np * (n - 1); ++j, e = fe_add(fe_sqr(e, P), fe_one(P), P)) fe_to_u64limbs(e, h_tails + 4 * j);
    for (uint32_t j = 0; j < k; ++j, e = fe_add(fe_sqr(e, P), fe_one(P), P)) h_coef[j] = mul29_prepare(e, P);
    PoolBlock d_coef, scratch0, out1, d_sums;
    FoldPlanHolder plan;
    ManySide side;
    DrainOnExit drain(c);
    std::function<int32_t()> once;
    const Fe s_inv = fe_inverse(h->shift, P);
    if (path == kMbPathOpen) {
        once = [&]() -> int32_t {
            OpenState st(c, h, np, 0, mlbatch_fuse_fold());   // its blocks go back stream-ordered and come out of the pool again on the next call
            MleHolder coeffs;
            ZKCHK(st.init(h_tails));
            ZKCHK(st.values());
            ZKCHK(st.combine(h_coef));
            for (uint32_t r = 1; r < n; ++r) {
                ZKCHK(st.fold_to(r, beta));
                ZKCHK(st.round(r, beta));
            }
            ZKCHK(st.fold_to(n, beta));
            return st.final_poly(coeffs);
        };
    } else if (path == kMbPathFused || path == kMbPathUnfused) {
        ZKCHK(d_coef.alloc(c, ml_scratch_bytes((size_t)k * sizeof(Mul29))));
        ZKCHK(out1.alloc(c, mle_block_bytes(n0 - 1)));
        ZKCHK(fri_fold_plan(c, n0, plan.put()));
        HIPCHK(hipMemcpyAsync(d_coef.p, h_coef, (size_t)k * sizeof(Mul29), hipMemcpyHostToDevice, c->stream));
        if (path == kMbPathUnfused) ZKCHK(scratch0.alloc(c, mle_block_bytes(n0)));
        once = [&]() -> int32_t {
            if (path == kMbPathFused) return combine_fold_launch(c, plan.get(), h->lde.as(), n0, k, d_coef.as<Mul29>(), s_inv, beta, out1.as());
            ZKCHK(lincomb_launch(c, h->codeword_ptrs(), k, d_coef.as<Mul29>(), scratch0.as(), 1ull << n0));
            return fri_fold2(c, plan.get(), scratch0.as(), n0, 0, s_inv, beta, out1.as());
        };
    } else {   // one round over the first table: the fold joined to the sums at kMlPointsPerPass points, in one pass or one pass per point
        ZKCHK(d_sums.alloc(c, ml_scratch_bytes((size_t)np * 64)));
        ZKCHK(side.init(c, n, h_tails, np));
        const bool fold = n >= 2;   // a table of one variable has nothing to fold into
        if (fold) ZKCHK(out1.alloc(c, mle_block_bytes(n - 1)));
        const uint32_t per_pass = path == kMbPathManyRound ? kMlPointsPerPass : 1;
        once = [&, fold, per_pass]() -> int32_t {
            for (uint32_t j0 = 0; j0 < np; j0 += per_pass)
                ZKCHK(side.pass(fold ? n - 1 : n, h->table(0), out1.as(), fold, beta, j0, per_pass, d_sums.as() + 8ull * j0));
            return ZK_OK;
        };
    }
    ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
    drain.armed = false;   // the span has waited for ev1
    return ZK_OK;
}
