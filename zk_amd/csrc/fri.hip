// fri.hip -- host side of the FRI low-degree proofs (kernels in fri_kernels.cuh; no reference item, definition: tests/fri_ref.py; DESIGN.md
// section 14): the coset LDE over zk_ntt, the fold by 2^a (one fused launch, or a binary launches behind ZK_FRI_FUSED_FOLD), the prover
// (per round: commit to the layer's 2^a column views, one host wait for the root, the host transcript, fold) and the host-only verifier.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "fri_kernels.cuh"

// ZK_FRI_FUSED_FOLD: 1 = a fold by 2^a is one launch of k_fri_fold<a>, 0 = a launches of k_fri_fold<1>.  The default is what
// profiles/fri.log shows faster at both 2^20 and 2^24 inputs for every arity.
constexpr uint32_t kFriFusedDefault = 1;
static bool fri_fused_fold() {
    static const bool fused = env_u64("ZK_FRI_FUSED_FOLD", kFriFusedDefault, 0, 1) != 0;
    return fused;
}
enum { kFriPathDefault = 0, kFriPathFused = 1, kFriPathBinary = 2 };
constexpr uint32_t kFriMaxBlowupLog = 8, kFriMaxQueries = 1024;

struct FriShape {
    uint32_t d, b, a, f, q, rounds;
    uint32_t log_m(uint32_t r) const { return d + b - a * r - a; }   // rows of layer r's commitment
};
// log_arity outside 1..3, log_blowup outside 1..8, n_queries outside 1..1024, log_final >= log_degree, log_arity not dividing
// log_degree - log_final (and a degree bound past the largest table) -> ZK_ERR_BAD_ARG
static int32_t fri_shape(uint32_t d, uint32_t b, uint32_t a, uint32_t f, uint32_t q, FriShape *sh) {
    if (a < 1 || a > kFriMaxArityLog || b < 1 || b > kFriMaxBlowupLog || q < 1 || q > kFriMaxQueries) return ZK_ERR_BAD_ARG;
    if (f >= d || (d - f) % a != 0 || d > kMaxVars) return ZK_ERR_BAD_ARG;
    *sh = {d, b, a, f, q, (d - f) / a};
    return ZK_OK;
}
static uint64_t fri_bytes(const FriShape &sh) {
    uint64_t per_query = 0;
    for (uint32_t r = 0; r < sh.rounds; ++r) per_query += (1ull << sh.a) + sh.log_m(r);
    return 32 * (sh.rounds + (1ull << sh.f) + sh.q * per_query);
}
// an element as it crosses the ABI (Montgomery limbs) that is fully reduced
bool zk::fri_elem(const uint64_t l[4], const FieldParams &P, Fe *out) {
    const Fe e = fe_from_u64limbs(l);
    Fe d;
    if (!sub8(d.v, e.v, P.p)) return false;   // not < p
    *out = e;
    return true;
}
static Fe fri_pow2k(Fe x, uint32_t k, const FieldParams &P) {   // x^(2^k)
    for (uint32_t i = 0; i < k; ++i) x = fe_sqr(x, P);
    return x;
}

// ---- the two-level power table of w^-1, w = root_of_unity(2^log_domain) ---------------------------------------------------------------
struct FriTables {
    PoolBlock lo, hi;
    FriTable t;
};
static int32_t fri_make_tables(zk_ctx *c, uint32_t log_domain, FriTables &T) {
    const FieldParams &P = c->fi->P;
    Fe w;
    if (!field_root_of_unity(*c->fi, log_domain, w)) return ZK_ERR_FFT_NO_ROOT;
    const uint32_t lo_bits = log_domain < kFriTableLoBits ? log_domain : kFriTableLoBits, hi_bits = log_domain - lo_bits;
    ZKCHK(T.lo.alloc(c, (size_t)32 << lo_bits));
    ZKCHK(T.hi.alloc(c, (size_t)32 << hi_bits));
    k_fri_tables<<<grid_for((1ull << lo_bits) + (1ull << hi_bits)), kBlock, 0, c->stream>>>(T.lo.as(), T.hi.as(), lo_bits, hi_bits, fe_inverse(w, P), P);
    HIPCHK(hipGetLastError());
    T.t = {T.lo.as(), T.hi.as(), lo_bits, hi_bits, 0};
    return ZK_OK;
}
// beta / s and w_{2^a}^-1, ^-2, ^-3 (fri_kernels.cuh), from beta and 1 / s
static FriConsts fri_consts(const FieldInfo &fi, uint32_t a, const Fe &s_inv, const Fe &beta) {
    const FieldParams &P = fi.P;
    FriConsts kc = {};
    kc.c = mul29_prepare(fe_mul(beta, s_inv, P), P);
    Fe w;
    field_root_of_unity(fi, a, w);
    const Fe w_inv = fe_pow_u64(w, (1ull << a) - 1, P);   // w_{2^a}^-1
    Fe cur = w_inv;
    for (uint32_t j = 1; j < (1u << (a - 1)); ++j) {
        kc.w[j - 1] = mul29_prepare(cur, P);
        cur = fe_mul(cur, w_inv, P);
    }
    return kc;
}
template <int A>
static void fri_launch(zk_ctx *c, const uint64_t *in, uint64_t *out, uint64_t M, const FriTable &tw, const FriConsts &kc) {
    if (M >= 64) {   // one 64-element run per wave, as the MSB fold is launched
        uint64_t g = M / kBlock;
        if (g > 2 * kMaxGridStream) g = 2 * kMaxGridStream;
        k_fri_fold<A, true><<<(uint32_t)(g ? g : 1), kBlock, 0, c->stream>>>(in, out, M, tw, kc, c->fi->P);
    } else {
        k_fri_fold<A, false><<<1, kBlock, 0, c->stream>>>(in, out, M, tw, kc, c->fi->P);
    }
}
// one layer: `in` of 2^n points over the coset of shift s (s_inv = 1 / s) -> `out` of 2^(n-a).  tw: the table with the layer's stride.
// The binary path keeps its a - 1 intermediate layers in `mid` (the caller's blocks, so that a timed loop allocates once).
struct FriMid {
    PoolBlock b[kFriMaxArityLog - 1];
};
static int32_t fri_mid_alloc(zk_ctx *c, uint32_t n, uint32_t a, FriMid &mid) {
    for (uint32_t l = 0; l + 1 < a; ++l) ZKCHK(mid.b[l].alloc(c, mle_block_bytes(n - 1 - l)));
    return ZK_OK;
}
static int32_t fri_fold_layer(zk_ctx *c, const uint64_t *in, uint32_t n, uint32_t a, const Fe &s_inv, const Fe &beta, FriTable tw, uint64_t *out,
                              bool fused, FriMid *mid) {
    const FieldParams &P = c->fi->P;
    if (fused || a == 1) {
        const FriConsts kc = fri_consts(*c->fi, a, s_inv, beta);
        const uint64_t M = 1ull << (n - a);
        if (a == 1) fri_launch<1>(c, in, out, M, tw, kc);
        else if (a == 2) fri_launch<2>(c, in, out, M, tw, kc);
        else fri_launch<3>(c, in, out, M, tw, kc);
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    Fe si = s_inv, bl = beta;
    const uint64_t *src = in;
    for (uint32_t l = 0; l < a; ++l) {   // fri_ref.fold's own order: (s, beta), (s^2, beta^2), (s^4, beta^4)
        uint64_t *dst = l + 1 == a ? out : mid->b[l].as();
        fri_launch<1>(c, src, dst, 1ull << (n - 1 - l), tw, fri_consts(*c->fi, 1, si, bl));
        src = dst;
        si = fe_sqr(si, P), bl = fe_sqr(bl, P);
        ++tw.stride_log;
    }
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// ---- what mlpcs.hip's opening takes of the rounds above: the table, one fold by 2, the gather's launch ------------------------------------
struct zk::FriFoldPlan {
    FriTables T;
};
int32_t zk::fri_fold_plan(zk_ctx *c, uint32_t log_domain, FriFoldPlan **out) {
    FriFoldPlan *pl = new (std::nothrow) FriFoldPlan();
    if (!pl) return ZK_ERR_ALLOC;
    const int32_t rc = fri_make_tables(c, log_domain, pl->T);
    if (rc != ZK_OK) {
        delete pl;
        return rc;
    }
    *out = pl;
    return ZK_OK;
}
void zk::fri_fold_plan_release(FriFoldPlan *pl) { delete pl; }   // the tables go back to the pool stream-ordered
void zk::fri_fold_plan_table(const FriFoldPlan *pl, const uint64_t **lo, const uint64_t **hi, uint32_t *lo_bits, uint32_t *hi_bits) {
    *lo = pl->T.t.lo, *hi = pl->T.t.hi, *lo_bits = pl->T.t.lo_bits, *hi_bits = pl->T.t.hi_bits;
}
int32_t zk::fri_fold2(zk_ctx *c, const FriFoldPlan *pl, const uint64_t *in, uint32_t n, uint32_t round, const Fe &s_inv, const Fe &beta, uint64_t *out) {
    FriTable tw = pl->T.t;
    tw.stride_log = round;
    return fri_fold_layer(c, in, n, 1, s_inv, beta, tw, out, true, nullptr);   // arity 2 is one launch on either setting of the switch
}
int32_t zk::fri_gather(zk_ctx *c, const uint64_t *layer, const uint64_t *tree, uint32_t log_m, uint32_t width, const uint64_t *d_idx, uint32_t n_queries,
                       uint64_t *rows, uint64_t *paths) {
    k_fri_gather<<<grid_for((uint64_t)n_queries * (width + log_m)), kBlock, 0, c->stream>>>(layer, tree, log_m, width, d_idx, n_queries, rows, paths);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// ---- the coset LDE: out[k] = sum_j c_j shift^j w^(j k) over 2^log_n points --------------------------------------------------------------
int32_t zk::fri_lde_into(zk_ctx *c, const zk_upoly *p, uint32_t log_n, const uint64_t shift[4], zk_mle *out) {
    const FieldParams &P = c->fi->P;
    MleHolder tmp;
    ZKCHK(mle_alloc(c, log_n, tmp.put()));
    const uint64_t n = 1ull << log_n;
    if (p->len) HIPCHK(hipMemcpyAsync(tmp->d, p->d, (size_t)p->len * 32, hipMemcpyDeviceToDevice, c->stream));
    if (p->len < n) HIPCHK(hipMemsetAsync(tmp->d + 4 * p->len, 0, (size_t)(n - p->len) * 32, c->stream));
    if (!fe_eq(fe_from_u64limbs(shift), fe_one(P))) {
        uint64_t one[4];
        fe_to_u64limbs(fe_one(P), one);
        ZKCHK(zk_mle_mul_powers(c, tmp.get(), shift, one));
    }
    return zk_ntt(c, tmp.get(), 0, out);   // tmp goes back to the pool stream-ordered
}

extern "C" int32_t zk_fri_lde(zk_ctx *c, const zk_upoly *p, uint32_t log_n, const uint64_t shift[4], zk_mle **out) {
    if (!c || !p || !shift || !out) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    Fe s;
    if (log_n > 63 || p->len > (1ull << log_n) || !fri_elem(shift, c->fi->P, &s) || fe_is_zero(s)) return ZK_ERR_BAD_ARG;
    if (log_n > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    ZKCHK(use_device(c));
    MleHolder res;
    ZKCHK(mle_alloc(c, log_n, res.put()));
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the blocks go back
    ZKCHK(fri_lde_into(c, p, log_n, shift, res.get()));
    drain.armed = false;
    *out = res.release();
    return ZK_OK;
}

extern "C" int32_t zk_fri_fold(zk_ctx *c, const zk_mle *in, uint32_t log_arity, const uint64_t shift[4], const uint64_t beta[4], zk_mle *out) {
    if (!c || !in || !shift || !beta || !out) return ZK_ERR_BAD_ARG;
    if (in->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const FieldParams &P = c->fi->P;
    Fe s, bt;
    if (log_arity < 1 || log_arity > kFriMaxArityLog) return ZK_ERR_BAD_ARG;
    if (!fri_elem(shift, P, &s) || fe_is_zero(s) || !fri_elem(beta, P, &bt)) return ZK_ERR_BAD_ARG;
    if (out == in || out->d == in->d) return ZK_ERR_BAD_ARG;
    if (in->n_vars >= log_arity && out->n_vars != in->n_vars - log_arity) return ZK_ERR_BAD_ARG;
    if (in->n_vars > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    if (in->n_vars < log_arity) return ZK_ERR_EVAL_LEN;
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)in->n_vars;
    const bool fused = fri_fused_fold();
    FriTables T;
    FriMid mid;
    DrainOnExit drain(c);
    ZKCHK(fri_make_tables(c, n, T));
    if (!fused) ZKCHK(fri_mid_alloc(c, n, log_arity, mid));
    ZKCHK(fri_fold_layer(c, in->d, n, log_arity, fe_inverse(s, P), bt, T.t, out->d, fused, &mid));
    drain.armed = false;   // enqueued: the blocks go back stream-ordered
    return ZK_OK;
}

extern "C" int32_t zk_fri_proof_bytes(uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final, uint32_t n_queries,
                                      uint64_t *out) {
    if (!out) return ZK_ERR_BAD_ARG;
    FriShape sh;
    ZKCHK(fri_shape(log_degree, log_blowup, log_arity, log_final, n_queries, &sh));
    *out = fri_bytes(sh);
    return ZK_OK;
}

// seed, the six parameters as 8-byte big-endian integers, be32(shift): what prover and verifier absorb first
static void fri_transcript_start(Sponge &sp, int32_t field, const FriShape &sh, const Fe &shift, const uint8_t seed[32], const FieldParams &P) {
    sp.init();
    sp.update(seed, 32);
    const uint64_t v[6] = {(uint64_t)field, sh.d, sh.b, sh.a, sh.f, sh.q};
    uint8_t be[48];
    for (int i = 0; i < 6; ++i)
        for (int k = 0; k < 8; ++k) be[8 * i + k] = (uint8_t)(v[i] >> (8 * (7 - k)));
    sp.update(be, 48);
    uint8_t sb[32];
    fe_to_bytes_be(shift, P, sb);
    sp.update(sb, 32);
}
uint64_t zk::fri_query_index(Sponge &sp, uint32_t log_m0) {
    uint8_t h[32];
    sp.sample_challenge(h);
    uint64_t v = 0;
    for (int k = 24; k < 32; ++k) v = (v << 8) | h[k];
    return v & ((1ull << log_m0) - 1);
}

extern "C" int32_t zk_fri_prove(zk_ctx *c, const zk_upoly *p, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final,
                                uint32_t n_queries, const uint64_t shift[4], const uint8_t seed[32], uint8_t *out_proof) {
    if (!c || !p || !shift || !seed || !out_proof) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    FriShape sh;
    Fe s;
    ZKCHK(fri_shape(log_degree, log_blowup, log_arity, log_final, n_queries, &sh));
    if (p->len > (1ull << sh.d) || !fri_elem(shift, c->fi->P, &s) || fe_is_zero(s)) return ZK_ERR_BAD_ARG;
    if (sh.d + sh.b > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    ZKCHK(use_device(c));
    MleHolder layer0;
    DrainOnExit drain(c);   // a call that leaves early waits for the stream before the layer goes back
    ZKCHK(mle_alloc(c, sh.d + sh.b, layer0.put()));
    ZKCHK(fri_lde_into(c, p, sh.d + sh.b, shift, layer0.get()));
    drain.armed = false;   // from here on the prover below waits on every path
    return fri_prove_layer0(c, log_degree, log_blowup, log_arity, log_final, n_queries, s, seed, layer0.get(), out_proof, nullptr, nullptr);
}

// The prover from a layer 0 it is given (zk_fri_prove: the LDE of its polynomial; pcs.hip: the DEEP quotient), which it reads and leaves
// intact.  out_idx (Q words, or null) receives the query indices idx_0.  `trace` (or null) names one more committed table in FRI's row
// layout: its rows and paths at the query indices are gathered by one more launch behind the layers' own and come back with the same
// download, in trace->staged (Q rows of `width` elements, Montgomery, then Q paths of log2 M_0 digests).  Waits for the stream on
// every path.
int32_t zk::fri_prove_layer0(zk_ctx *c, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final, uint32_t n_queries,
                             const Fe &s, const uint8_t seed[32], const zk_mle *layer0, uint8_t *out_proof, uint64_t *out_idx, FriTraceOpen *trace) {
    const FieldParams &P = c->fi->P;
    FriShape sh;
    ZKCHK(fri_shape(log_degree, log_blowup, log_arity, log_final, n_queries, &sh));
    const uint32_t n0 = sh.d + sh.b, a = sh.a, R = sh.rounds, Q = sh.q;
    // owners first, the drain last: a call that leaves early waits for the stream before any block goes back
    std::vector<MleHolder> layers;   // layers[r], r >= 1 (layer 0 is the caller's)
    std::vector<const uint64_t *> layer_at;
    std::vector<PoolBlock> trees;
    std::vector<uint64_t> idx, staged;
    try {
        layers.resize(R + 1);
        layer_at.resize(R + 1);
        trees.resize(R);
        idx.resize(Q);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    FriTables T;
    FriMid mid;
    PoolBlock d_idx, d_stage;
    MleHolder coeffs;
    DrainOnExit drain(c);
    const bool fused = fri_fused_fold();

    layer_at[0] = layer0->d;
    ZKCHK(fri_make_tables(c, n0, T));
    if (!fused) ZKCHK(fri_mid_alloc(c, n0, a, mid));   // the largest layer's: the later layers fit in them
    Sponge sp;
    fri_transcript_start(sp, c->field, sh, s, seed, P);
    Fe s_inv = fe_inverse(s, P);
    uint8_t *at = out_proof;
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t n = n0 - a * r, m = n - a;
        ZKCHK(trees[r].alloc(c, (size_t)64 << m));
        const uint64_t *cols[1 << kFriMaxArityLog];
        for (uint32_t j = 0; j < (1u << a); ++j) cols[j] = layer_at[r] + 4 * ((uint64_t)j << m);   // column j = v[j M : (j + 1) M]
        ZKCHK(merkle_build_raw(c, cols, 1u << a, m, trees[r].as()));
        const uint64_t *root = trees[r].as() + 4 * ((2ull << m) - 2);
        HIPCHK(hipMemcpyAsync(c->h_pinned, root, 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));   // the round's one host wait
        memcpy(at, c->h_pinned, 32);
        sp.update(at, 32);
        at += 32;
        const Fe beta = squeeze_field_element(sp, P);
        ZKCHK(mle_alloc(c, m, layers[r + 1].put()));
        layer_at[r + 1] = layers[r + 1]->d;
        FriTable tw = T.t;
        tw.stride_log = a * r;
        ZKCHK(fri_fold_layer(c, layer_at[r], n, a, s_inv, beta, tw, layers[r + 1]->d, fused, &mid));
        s_inv = fri_pow2k(s_inv, a, P);
    }
    // the final polynomial: inverse transform of layer R over its coset, first 2^f coefficients
    const uint32_t nR = sh.f + sh.b;
    const uint64_t n_final = 1ull << sh.f;
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
    // the queries: every layer opened for all of them with one gather launch, one download
    for (uint32_t q = 0; q < Q; ++q) idx[q] = fri_query_index(sp, sh.log_m(0));
    if (out_idx) memcpy(out_idx, idx.data(), (size_t)Q * 8);
    uint64_t per_query = 0;
    for (uint32_t r = 0; r < R; ++r) per_query += (1ull << a) + sh.log_m(r);
    const uint64_t trace_items = trace ? (uint64_t)Q * (trace->width + sh.log_m(0)) : 0;   // behind the layers' in the staging block
    try {
        staged.resize(4 * Q * per_query);
        if (trace) trace->staged.resize(4 * trace_items);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    size_t idx_bytes = 32, stage_bytes = 32;
    while (idx_bytes < (size_t)Q * 8) idx_bytes <<= 1;
    while (stage_bytes < (size_t)(Q * per_query + trace_items) * 32) stage_bytes <<= 1;
    ZKCHK(d_idx.alloc(c, idx_bytes));
    ZKCHK(d_stage.alloc(c, stage_bytes));
    HIPCHK(hipMemcpyAsync(d_idx.p, idx.data(), (size_t)Q * 8, hipMemcpyHostToDevice, c->stream));
    uint64_t off = 0;   // in elements of the staging block: layer r's rows, then its paths
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t m = sh.log_m(r);
        uint64_t *rows = d_stage.as() + 4 * off, *paths = rows + 4 * ((uint64_t)Q << a);
        k_fri_gather<<<grid_for((uint64_t)Q * ((1u << a) + m)), kBlock, 0, c->stream>>>(layer_at[r], trees[r].as(), m, 1u << a, d_idx.as(), Q, rows, paths);
        off += (uint64_t)Q * ((1ull << a) + m);
    }
    if (trace) {   // the same indices, the same row layout: M_0 rows of `width` columns at stride M_0
        uint64_t *rows = d_stage.as() + 4 * off, *paths = rows + 4 * (uint64_t)Q * trace->width;
        k_fri_gather<<<grid_for(trace_items), kBlock, 0, c->stream>>>(trace->table, trace->tree, sh.log_m(0), trace->width, d_idx.as(), Q, rows, paths);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(staged.data(), d_stage.p, (size_t)Q * per_query * 32, hipMemcpyDeviceToHost, c->stream));
    if (trace) HIPCHK(hipMemcpyAsync(trace->staged.data(), d_stage.as() + 4 * off, (size_t)trace_items * 32, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    for (uint32_t q = 0; q < Q; ++q) {
        off = 0;
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t m = sh.log_m(r);
            const uint64_t *rows = staged.data() + 4 * (off + ((uint64_t)q << a));
            const uint64_t *paths = staged.data() + 4 * (off + ((uint64_t)Q << a) + (uint64_t)q * m);
            for (uint32_t j = 0; j < (1u << a); ++j, at += 32) fe_to_bytes_be(fe_from_u64limbs(rows + 4 * j), P, at);
            memcpy(at, paths, (size_t)m * 32);
            at += (size_t)m * 32;
            off += (uint64_t)Q * ((1ull << a) + m);
        }
    }
    return ZK_OK;
}

// ---- the verifier: host only, no context --------------------------------------------------------------------------------------------------
// a 32-byte big-endian canonical integer -> Montgomery element; false when it is not below p
bool zk::fri_from_be32(const uint8_t *b, const FieldParams &P, Fe *out) {
    uint64_t l[4];
    for (int i = 0; i < 4; ++i) {
        uint64_t v = 0;
        for (int k = 0; k < 8; ++k) v = (v << 8) | b[8 * (3 - i) + k];
        l[i] = v;
    }
    const Fe e = fe_from_u64limbs(l);
    Fe d;
    if (!sub8(d.v, e.v, P.p)) return false;
    *out = fe_from_canonical(e, P);
    return true;
}
// fri_ref.fold(row, x, beta, a)[0] with 1 / x given: the row is its own coset of 2^a points
Fe zk::fri_fold_row(Fe *v, uint32_t a, Fe x_inv, Fe beta, const Fe &half, const FieldInfo &fi) {
    const FieldParams &P = fi.P;
    for (uint32_t l = 0; l < a; ++l) {
        const uint32_t n = 1u << (a - l), h = n / 2;
        Fe w;
        field_root_of_unity(fi, a - l, w);
        const Fe w_inv = fe_pow_u64(w, n - 1, P);
        Fe cur = fe_mul(half, x_inv, P);   // 1 / (2 x w^i)
        for (uint32_t i = 0; i < h; ++i) {
            const Fe sum = fe_mul(fe_add(v[i], v[i + h], P), half, P);
            v[i] = fe_add(sum, fe_mul(fe_mul(beta, fe_sub(v[i], v[i + h], P), P), cur, P), P);
            cur = fe_mul(cur, w_inv, P);
        }
        x_inv = fe_sqr(x_inv, P), beta = fe_sqr(beta, P);
    }
    return v[0];
}

extern "C" int32_t zk_fri_verify_host(int32_t field, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final,
                                      uint32_t n_queries, const uint64_t shift[4], const uint8_t seed[32], const uint8_t *proof, uint64_t proof_len,
                                      int32_t *out_ok) {
    return fri_verify_core(field, log_degree, log_blowup, log_arity, log_final, n_queries, shift, seed, proof, proof_len, out_ok, nullptr);
}
// zk_fri_verify_host itself; out_idx (Q words, or null) receives the query indices idx_0 of an accepted proof (pcs.hip checks its
// commitment's rows against the round-0 rows at them)
int32_t zk::fri_verify_core(int32_t field, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final, uint32_t n_queries,
                            const uint64_t shift[4], const uint8_t seed[32], const uint8_t *proof, uint64_t proof_len, int32_t *out_ok,
                            uint64_t *out_idx) {
    if (!shift || !seed || !proof || !out_ok) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    FriShape sh;
    Fe s0;
    ZKCHK(fri_shape(log_degree, log_blowup, log_arity, log_final, n_queries, &sh));
    if (!fri_elem(shift, P, &s0) || fe_is_zero(s0) || proof_len != fri_bytes(sh)) return ZK_ERR_BAD_ARG;
    const uint32_t n0 = sh.d + sh.b, a = sh.a, R = sh.rounds, width = 1u << a;
    if (n0 > fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    *out_ok = 0;
    Sponge sp;
    fri_transcript_start(sp, field, sh, s0, seed, P);
    std::vector<Fe> beta(R), s_inv(R), w_inv(R), final_co((size_t)1 << sh.f);
    Fe s = s0;
    for (uint32_t r = 0; r < R; ++r) {
        sp.update(proof + 32 * r, 32);
        beta[r] = squeeze_field_element(sp, P);
        Fe w;
        field_root_of_unity(*fi, n0 - a * r, w);
        s_inv[r] = fe_inverse(s, P);
        w_inv[r] = fe_inverse(w, P);
        s = fri_pow2k(s, a, P);
    }
    const uint8_t *at = proof + 32 * (size_t)R;
    for (size_t j = 0; j < final_co.size(); ++j)
        if (!fri_from_be32(at + 32 * j, P, &final_co[j])) return ZK_OK;   // not canonical: a verdict, not an error
    sp.update(at, 32 * final_co.size());
    at += 32 * final_co.size();
    Fe w_last;   // layer R: N_R = M_{R-1} points over the coset of s (= s_R by now)
    field_root_of_unity(*fi, sh.log_m(R - 1), w_last);
    const Fe half = fe_inverse(fe_from_u32(2, P), P);
    for (uint32_t q = 0; q < sh.q; ++q) {
        uint64_t idx = fri_query_index(sp, sh.log_m(0));
        if (out_idx) out_idx[q] = idx;
        Fe y = fe_zero();
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t m = sh.log_m(r);
            const uint64_t rho = idx & ((1ull << m) - 1);
            Fe row[1 << kFriMaxArityLog];
            uint64_t limbs[4 << kFriMaxArityLog];
            for (uint32_t j = 0; j < width; ++j) {
                if (!fri_from_be32(at + 32 * j, P, &row[j])) return ZK_OK;
                fe_to_u64limbs(row[j], limbs + 4 * j);
            }
            at += 32 * (size_t)width;
            int32_t ok = 0;
            ZKCHK(zk_merkle_verify_host(field, proof + 32 * (size_t)r, m, width, rho, limbs, at, &ok));
            at += 32 * (size_t)m;
            if (!ok) return ZK_OK;
            if (r > 0 && !fe_eq(row[idx >> m], y)) return ZK_OK;
            const Fe x_inv = fe_mul(s_inv[r], fe_pow_u64(w_inv[r], rho, P), P);
            y = fri_fold_row(row, a, x_inv, beta[r], half, *fi);
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

// device time of `reps` folds of `in` by 2^log_arity into `out` between two HIP events after as many untimed ones (the power table, the
// constants and the binary path's intermediate layers are made once, outside): path 0 = as the switch decides, 1 = the fused kernel,
// 2 = log_arity launches of k_fri_fold<1>
extern "C" int32_t zk_bench_fri_fold(zk_ctx *c, const zk_mle *in, uint32_t log_arity, zk_mle *out, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !in || !out || !out_ms || reps < 1 || path < 0 || path > 2) return ZK_ERR_BAD_ARG;
    if (in->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (log_arity < 1 || log_arity > kFriMaxArityLog || out == in || out->d == in->d) return ZK_ERR_BAD_ARG;
    if (in->n_vars >= log_arity && out->n_vars != in->n_vars - log_arity) return ZK_ERR_BAD_ARG;
    if (in->n_vars > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    if (in->n_vars < log_arity) return ZK_ERR_EVAL_LEN;
    ZKCHK(use_device(c));
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)in->n_vars;
    const bool fused = path == kFriPathDefault ? fri_fused_fold() : path == kFriPathFused;
    const Fe s_inv = fe_inverse(fe_from_u32(c->fi->generator, P), P), beta = c->fi->two_adic_root;   // any non-zero pair
    FriTables T;
    FriMid mid;
    DrainOnExit drain(c);   // the tables' kernels: a failed allocation after them waits before the tables' block goes back
    ZKCHK(fri_make_tables(c, n, T));
    if (!fused) ZKCHK(fri_mid_alloc(c, n, log_arity, mid));
    auto once = [&] { return fri_fold_layer(c, in->d, n, log_arity, s_inv, beta, T.t, out->d, fused, &mid); };
    ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
    drain.armed = false;   // the span has waited for ev1
    return ZK_OK;
}
