// pcs.hip -- host side of the FRI polynomial commitment (kernels in pcs_kernels.cuh; no reference item, definition: tests/pcs_ref.py;
// DESIGN.md section 15): the DEEP quotient over the extension domain, the commitment handle (the k LDE tables, their tree in FRI's row
// layout, a copy of the coefficients), the opening at a point (values, host transcript, quotient, fri.hip's prover on it with the
// commitment's rows and paths gathered behind the prover's own) and the host-only verifier over fri.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "pcs_kernels.cuh"

constexpr uint32_t kPcsMaxColumns = 1024;   // the Merkle leaf's column limit (merkle_kernels.cuh kMerkleMaxColumns)
constexpr uint32_t kPcsMaxArityLog = 3, kPcsMaxBlowupLog = 8, kPcsMaxQueries = 1024;   // FRI's limits (fri.hip)

struct zk_pcs {
    zk_ctx *ctx;
    uint32_t k, d, b, a;
    Fe shift;
    PoolBlock lde;      // F_0 | F_1 | ... | F_{k-1}, 2^(d+b) elements each: column c 2^a + j of the tree is at stride M, as a FRI layer's are
    PoolBlock tree;     // every level over M = 2^(d+b-a) rows of k 2^a columns
    PoolBlock coeffs;   // k x 2^d coefficients, zero padded
};
static void pcs_release(zk_pcs *h) { delete h; }   // the blocks go back to the pool with their owner
using PcsHolder = Scoped<zk_pcs, pcs_release>;

static size_t scratch_bytes(size_t bytes) {
    size_t b = 32;
    while (b < bytes) b <<= 1;
    return b;
}
static Fe pow2k(Fe x, uint32_t k, const FieldParams &P) {   // x^(2^k)
    for (uint32_t i = 0; i < k; ++i) x = fe_sqr(x, P);
    return x;
}
// z^N == s^N: z is one of the N points s w^i (the host's two exponentiations)
static bool on_domain(const Fe &s, const Fe &z, uint32_t log_n, const FieldParams &P) { return fe_eq(pow2k(z, log_n, P), pow2k(s, log_n, P)); }
// d, b, a as FRI takes them and the column limit
static bool commit_shape(uint64_t k, uint32_t d, uint32_t b, uint32_t a) {
    return k >= 1 && a >= 1 && a <= kPcsMaxArityLog && b >= 1 && b <= kPcsMaxBlowupLog && d >= a && d <= kMaxVars && (k << a) <= kPcsMaxColumns;
}
static bool open_shape(uint32_t d, uint32_t a, uint32_t f, uint32_t q) { return q >= 1 && q <= kPcsMaxQueries && f < d && (d - f) % a == 0; }
static void fe_to_be32(const uint64_t *limbs, const FieldParams &P, uint8_t *out) { fe_to_bytes_be(fe_from_u64limbs(limbs), P, out); }

// alpha and fri_seed: seed; be64 of field id, k, d, b, a, f, Q; be32(shift); root; be32(z); be32(y_0) .. be32(y_{k-1})
static void pcs_challenges(int32_t field, uint32_t k, uint32_t d, uint32_t b, uint32_t a, uint32_t f, uint32_t q, const Fe &shift, const uint8_t seed[32],
                           const uint8_t root[32], const Fe &z, const Fe *ys, const FieldParams &P, Fe *alpha, uint8_t fri_seed[32]) {
    Sponge sp;
    sp.init();
    sp.update(seed, 32);
    const uint64_t v[7] = {(uint64_t)field, k, d, b, a, f, q};
    uint8_t be[56];
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 8; ++j) be[8 * i + j] = (uint8_t)(v[i] >> (8 * (7 - j)));
    sp.update(be, 56);
    uint8_t eb[32];
    fe_to_bytes_be(shift, P, eb);
    sp.update(eb, 32);
    sp.update(root, 32);
    fe_to_bytes_be(z, P, eb);
    sp.update(eb, 32);
    for (uint32_t c = 0; c < k; ++c) {
        fe_to_bytes_be(ys[c], P, eb);
        sp.update(eb, 32);
    }
    *alpha = squeeze_field_element(sp, P);
    sp.sample_challenge(fri_seed);
}
// Y = sum_c alpha^c y_c (Horner)
static Fe combine_values(const Fe *ys, uint32_t k, const Fe &alpha, const FieldParams &P) {
    Fe y = ys[k - 1];
    for (uint32_t c = k - 1; c-- > 0;) y = fe_add(fe_mul(y, alpha, P), ys[c], P);
    return y;
}

// ---- the quotient --------------------------------------------------------------------------------------------------------------------
// what one size needs beside the columns: the power table of s w^i and the device array of the k column pointers.  Enqueues only.
struct QuotientPlan {
    PcsTable tb;
    const uint64_t *const *cols;
    uint64_t *totals, *inv;
};
static int32_t quotient_plan(zk_ctx *c, PoolScope &ps, const uint64_t *const *cols, uint32_t k, uint32_t n, const Fe &s, QuotientPlan *pl) {
    const FieldParams &P = c->fi->P;
    Fe w;
    if (!field_root_of_unity(*c->fi, n, w)) return ZK_ERR_FFT_NO_ROOT;
    const uint32_t lo_bits = n < kPcsTableLoBits ? n : kPcsTableLoBits, hi_bits = n - lo_bits;
    uint64_t *lo = nullptr, *hi = nullptr;
    const uint64_t **table = nullptr;
    ZKCHK(ps.get((size_t)32 << lo_bits, &lo));
    ZKCHK(ps.get((size_t)32 << hi_bits, &hi));
    ZKCHK(ps.get(scratch_bytes((size_t)k * sizeof(uint64_t *)), &table));
    pl->totals = pl->inv = nullptr;
    const uint64_t N = 1ull << n;
    if (N > kPcsChunk) {
        ZKCHK(ps.get(scratch_bytes((size_t)(N / kPcsChunk) * 32), &pl->totals));
        ZKCHK(ps.get(scratch_bytes((size_t)(N / kPcsChunk) * 32), &pl->inv));
    }
    k_pcs_tables<<<grid_for((1ull << lo_bits) + (1ull << hi_bits)), kBlock, 0, c->stream>>>(lo, hi, lo_bits, hi_bits, w, s, P);
    for (uint32_t base = 0; base < k; base += kPcsPtrBatch) {
        PcsPtrs bt = {};
        const uint32_t count = k - base < kPcsPtrBatch ? k - base : kPcsPtrBatch;
        for (uint32_t j = 0; j < count; ++j) bt.p[j] = cols[base + j];
        k_pcs_put_ptrs<<<1, 64, 0, c->stream>>>(table, base, count, bt);
    }
    HIPCHK(hipGetLastError());
    pl->tb = {lo, hi, lo_bits, hi_bits};
    pl->cols = table;
    return ZK_OK;
}
// out[i] = (sum_c alpha^c cols[c][i] - y) / (s w^i - z) over 2^n points, times s w^i when times_x: one launch up to one chunk, three
// above.  Enqueues only.
static int32_t quotient_launch(zk_ctx *c, const QuotientPlan &pl, uint32_t k, uint32_t n, const Fe &z, const Fe &y, const Fe &alpha, uint64_t *out,
                               bool times_x = false) {
    const FieldParams &P = c->fi->P;
    const uint64_t N = 1ull << n;
    const PcsConsts kc = {z, y, mul29_prepare(alpha, P)};
    const uint64_t nc = N / kPcsChunk;   // one workgroup per chunk, no loop: every output has exactly one writer at every size
    if (nc > 0x7fffffffull) return ZK_ERR_UNSUPPORTED;
    if (N > kPcsChunk) {
        k_pcs_chunk_products<<<(uint32_t)nc, kBlock, 0, c->stream>>>(N, pl.tb, z, P, pl.totals);
        k_pcs_totals<<<1, kBlock, 0, c->stream>>>(pl.totals, nc, P, pl.inv);
    }
    auto apply = [&](auto alone, auto run, auto tx) {
        k_pcs_apply<decltype(alone)::value, decltype(run)::value, decltype(tx)::value>
            <<<decltype(alone)::value ? 1u : (uint32_t)nc, kBlock, 0, c->stream>>>(pl.cols, k, N, pl.tb, kc, P, pl.inv, out);
    };
    auto pick = [&](auto tx) {
        if (N > kPcsChunk) apply(std::false_type{}, std::true_type{}, tx);
        else if (N >= 64) apply(std::true_type{}, std::true_type{}, tx);
        else apply(std::true_type{}, std::false_type{}, tx);
    };
    if (times_x) pick(std::true_type{});
    else pick(std::false_type{});
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// NULLs and n_columns == 0 -> BAD_ARG; another context's handle -> CONTEXT_MISMATCH; then the shapes -> BAD_ARG
static int32_t quotient_columns(const zk_ctx *c, const zk_mle *const *columns, uint32_t k, const zk_mle *out) {
    if (!c || !columns || k == 0 || !out) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (!columns[j]) return ZK_ERR_BAD_ARG;
    if (out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    for (uint32_t j = 0; j < k; ++j)
        if (columns[j]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (k > kPcsMaxColumns) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (columns[j]->n_vars != out->n_vars || columns[j] == out || columns[j]->d == out->d) return ZK_ERR_BAD_ARG;
    return ZK_OK;
}

extern "C" int32_t zk_deep_quotient(zk_ctx *c, const zk_mle *const *columns, uint32_t n_columns, const uint64_t shift[4], const uint64_t z[4],
                                    const uint64_t *values, const uint64_t alpha[4], zk_mle *out) {
    if (!shift || !z || !values || !alpha) return ZK_ERR_BAD_ARG;
    ZKCHK(quotient_columns(c, columns, n_columns, out));
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)out->n_vars;
    Fe s, zf, al;
    if (!fri_elem(shift, P, &s) || fe_is_zero(s) || !fri_elem(z, P, &zf) || !fri_elem(alpha, P, &al)) return ZK_ERR_BAD_ARG;
    std::vector<Fe> ys;
    try {
        ys.resize(n_columns);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (uint32_t j = 0; j < n_columns; ++j)
        if (!fri_elem(values + 4 * j, P, &ys[j])) return ZK_ERR_BAD_ARG;
    if (on_domain(s, zf, n, P)) return ZK_ERR_BAD_ARG;
    if (n > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    ZKCHK(use_device(c));
    std::vector<const uint64_t *> cols;
    try {
        cols.resize(n_columns);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (uint32_t j = 0; j < n_columns; ++j) cols[j] = columns[j]->d;
    PoolScope ps(c);
    QuotientPlan pl;
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the blocks go back
    ZKCHK(quotient_plan(c, ps, cols.data(), n_columns, n, s, &pl));
    ZKCHK(quotient_launch(c, pl, n_columns, n, zf, combine_values(ys.data(), n_columns, al, P), al, out->d));
    drain.armed = false;   // enqueued: the blocks go back stream-ordered
    return ZK_OK;
}

// ---- the commitment ------------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_pcs_commit(zk_ctx *c, const zk_upoly *const *polys, uint32_t k, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity,
                                 const uint64_t shift[4], zk_pcs **out) {
    if (!c || !polys || k == 0 || !shift || !out) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (!polys[j]) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (polys[j]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const FieldParams &P = c->fi->P;
    const uint32_t d = log_degree, b = log_blowup, a = log_arity;
    Fe s;
    if (!commit_shape(k, d, b, a) || !fri_elem(shift, P, &s) || fe_is_zero(s)) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (polys[j]->len > (1ull << d)) return ZK_ERR_BAD_ARG;
    const uint32_t n0 = d + b, m = n0 - a;
    if (n0 > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    ZKCHK(use_device(c));
    PcsHolder h(new (std::nothrow) zk_pcs());
    if (!h.get()) return ZK_ERR_ALLOC;
    h->ctx = c, h->k = k, h->d = d, h->b = b, h->a = a, h->shift = s;
    std::vector<const uint64_t *> cols;
    try {
        cols.resize((size_t)k << a);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the blocks go back
    ZKCHK(h->lde.alloc(c, scratch_bytes(((size_t)k * 32) << n0)));
    ZKCHK(h->tree.alloc(c, (size_t)64 << m));
    ZKCHK(h->coeffs.alloc(c, scratch_bytes(((size_t)k * 32) << d)));
    HIPCHK(hipMemsetAsync(h->coeffs.p, 0, ((size_t)k * 32) << d, c->stream));
    for (uint32_t j = 0; j < k; ++j) {
        zk_mle view = {c, n0, h->lde.as() + 4 * ((uint64_t)j << n0)};   // F_j, a table of its own to the LDE
        ZKCHK(fri_lde_into(c, polys[j], n0, shift, &view));
        if (polys[j]->len)
            HIPCHK(hipMemcpyAsync(h->coeffs.as() + 4 * ((uint64_t)j << d), polys[j]->d, (size_t)polys[j]->len * 32, hipMemcpyDeviceToDevice, c->stream));
        for (uint32_t i = 0; i < (1u << a); ++i) cols[((size_t)j << a) + i] = view.d + 4 * ((uint64_t)i << m);   // column j 2^a + i = F_j[i M : (i + 1) M]
    }
    ZKCHK(merkle_build_raw(c, cols.data(), k << a, m, h->tree.as()));
    drain.armed = false;
    *out = h.release();
    return ZK_OK;
}
extern "C" int32_t zk_pcs_free(zk_pcs *h) {
    pcs_release(h);   // back to its context's pool; reuse is stream-ordered
    return ZK_OK;
}
extern "C" int32_t zk_pcs_n_polys(const zk_pcs *h, uint32_t *out) {
    if (!h || !out) return ZK_ERR_BAD_ARG;
    *out = h->k;
    return ZK_OK;
}
extern "C" int32_t zk_pcs_root(zk_ctx *c, const zk_pcs *h, uint8_t out[32]) {
    if (!c || !h || !out) return ZK_ERR_BAD_ARG;
    if (h->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    const uint32_t m = h->d + h->b - h->a;
    HIPCHK(hipMemcpyAsync(out, h->tree.as() + 4 * ((2ull << m) - 2), 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
extern "C" int32_t zk_pcs_proof_bytes(uint32_t k, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final, uint32_t n_queries,
                                      uint64_t *out) {
    if (!out) return ZK_ERR_BAD_ARG;
    if (!commit_shape(k, log_degree, log_blowup, log_arity) || !open_shape(log_degree, log_arity, log_final, n_queries)) return ZK_ERR_BAD_ARG;
    uint64_t fri = 0;
    ZKCHK(zk_fri_proof_bytes(log_degree, log_blowup, log_arity, log_final, n_queries, &fri));
    *out = fri + 32ull * n_queries * (((uint64_t)k << log_arity) + log_degree + log_blowup - log_arity);
    return ZK_OK;
}

// ---- the opening ---------------------------------------------------------------------------------------------------------------------
// one host wait before the prover's own: for the values and the root (a single download); the quotient and the openings add none
extern "C" int32_t zk_pcs_open(zk_ctx *c, const zk_pcs *h, const uint64_t z[4], uint32_t log_final, uint32_t n_queries, const uint8_t seed[32],
                               uint64_t *out_values, uint8_t *out_proof) {
    if (!c || !h || !z || !seed || !out_values || !out_proof) return ZK_ERR_BAD_ARG;
    if (h->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const FieldParams &P = c->fi->P;
    const uint32_t k = h->k, d = h->d, b = h->b, a = h->a, f = log_final, Q = n_queries, n0 = d + b, m = n0 - a, width = k << a;
    Fe zf;
    if (!open_shape(d, a, f, Q) || !fri_elem(z, P, &zf) || on_domain(h->shift, zf, n0, P)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    std::vector<Fe> ys;
    std::vector<uint64_t> vals;
    std::vector<const uint64_t *> cols;
    try {
        ys.resize(k);
        vals.resize((size_t)4 * k + 4);
        cols.resize(k);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    uint64_t fri_bytes = 0;
    ZKCHK(zk_fri_proof_bytes(d, b, a, f, Q, &fri_bytes));
    MleHolder quo;
    PoolScope ps(c);
    DrainOnExit drain(c);   // owners first, the drain last: a call that leaves early waits before any block goes back
    // the k values and the root: two launches for all polynomials, one download, the opening's first host wait
    const uint32_t per_poly = (uint32_t)std::min<uint64_t>(((1ull << d) + kBlock * kPcsEvalRun - 1) / (kBlock * kPcsEvalRun), kPcsEvalMaxBlocks);
    uint64_t *d_part = nullptr, *d_vals = nullptr;
    ZKCHK(ps.get(scratch_bytes((size_t)k * per_poly * 32), &d_part));
    ZKCHK(ps.get(scratch_bytes((size_t)(k + 1) * 32), &d_vals));
    k_pcs_eval_partial<<<dim3(per_poly, k), kBlock, 0, c->stream>>>(h->coeffs.as(), d, zf, P, d_part);
    k_pcs_eval_final<<<k, kBlock, 0, c->stream>>>(d_part, per_poly, P, d_vals);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d_vals + 4 * (size_t)k, h->tree.as() + 4 * ((2ull << m) - 2), 32, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(vals.data(), d_vals, (size_t)(k + 1) * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t j = 0; j < k; ++j) ys[j] = fe_from_u64limbs(vals.data() + 4 * j);
    Fe alpha;
    uint8_t fri_seed[32];
    pcs_challenges(c->field, k, d, b, a, f, Q, h->shift, seed, reinterpret_cast<const uint8_t *>(vals.data() + 4 * (size_t)k), zf, ys.data(), P, &alpha, fri_seed);
    // the quotient, then the shared prover on it with the commitment's rows and paths joined to its final download
    ZKCHK(mle_alloc(c, n0, quo.put()));
    for (uint32_t j = 0; j < k; ++j) cols[j] = h->lde.as() + 4 * ((uint64_t)j << n0);
    QuotientPlan pl;
    ZKCHK(quotient_plan(c, ps, cols.data(), k, n0, h->shift, &pl));
    // layer 0 is x_i q[i]: X q(X) has at most 2^d coefficients only if q has at most 2^d - 1, which is what a committed f_c of at most
    // 2^d coefficients gives; q itself would let one more coefficient through
    ZKCHK(quotient_launch(c, pl, k, n0, zf, combine_values(ys.data(), k, alpha, P), alpha, quo->d, true));
    FriTraceOpen trace = {h->lde.as(), h->tree.as(), width, {}};
    drain.armed = false;   // the prover waits on every path
    ZKCHK(fri_prove_layer0(c, d, b, a, f, Q, h->shift, fri_seed, quo.get(), out_proof, nullptr, &trace));
    uint8_t *at = out_proof + fri_bytes;
    const uint64_t *rows = trace.staged.data(), *paths = rows + 4 * (size_t)Q * width;
    for (uint32_t q = 0; q < Q; ++q) {
        for (uint32_t j = 0; j < width; ++j, at += 32) fe_to_be32(rows + 4 * ((size_t)q * width + j), P, at);
        memcpy(at, paths + 4 * (size_t)q * m, (size_t)m * 32);
        at += (size_t)m * 32;
    }
    memcpy(out_values, vals.data(), (size_t)k * 32);
    return ZK_OK;
}

// ---- the verifier: host only, no context -----------------------------------------------------------------------------------------------
extern "C" int32_t zk_pcs_verify_host(int32_t field, uint32_t k, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final,
                                      uint32_t n_queries, const uint64_t shift[4], const uint8_t seed[32], const uint8_t root[32], const uint64_t z[4],
                                      const uint64_t *values, const uint8_t *proof, uint64_t proof_len, int32_t *out_ok) {
    if (!shift || !seed || !root || !z || !values || !proof || !out_ok) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    const uint32_t d = log_degree, b = log_blowup, a = log_arity, f = log_final, Q = n_queries;
    uint64_t want_len = 0;
    ZKCHK(zk_pcs_proof_bytes(k, d, b, a, f, Q, &want_len));
    Fe s, zf;
    if (!fri_elem(shift, P, &s) || fe_is_zero(s) || !fri_elem(z, P, &zf) || proof_len != want_len) return ZK_ERR_BAD_ARG;
    std::vector<Fe> ys, row;
    std::vector<uint64_t> idx, limbs;
    const uint32_t n0 = d + b, m = n0 - a, width = k << a, R = (d - f) / a;
    try {
        ys.resize(k);
        row.resize(width);
        limbs.resize((size_t)4 * width);
        idx.resize(Q);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (uint32_t j = 0; j < k; ++j)
        if (!fri_elem(values + 4 * j, P, &ys[j])) return ZK_ERR_BAD_ARG;
    if (on_domain(s, zf, n0, P)) return ZK_ERR_BAD_ARG;
    if (n0 > fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    Fe alpha;
    uint8_t fri_seed[32];
    pcs_challenges(field, k, d, b, a, f, Q, s, seed, root, zf, ys.data(), P, &alpha, fri_seed);
    uint64_t fri_len = 0;
    ZKCHK(zk_fri_proof_bytes(d, b, a, f, Q, &fri_len));
    int32_t ok = 0;
    ZKCHK(fri_verify_core(field, d, b, a, f, Q, shift, fri_seed, proof, fri_len, &ok, idx.data()));
    *out_ok = 0;
    if (!ok) return ZK_OK;
    Fe w;
    field_root_of_unity(*fi, n0, w);
    const Fe y_comb = combine_values(ys.data(), k, alpha, P);
    const uint64_t per_query = (fri_len / 32 - R - (1ull << f)) / Q;   // elements of one query's part of the FRI proof; its round-0 row is first
    const uint8_t *at = proof + fri_len;
    for (uint32_t q = 0; q < Q; ++q) {
        for (uint32_t j = 0; j < width; ++j) {
            if (!fri_from_be32(at + 32 * (size_t)j, P, &row[j])) return ZK_OK;   // not canonical: a verdict, not an error
            fe_to_u64limbs(row[j], limbs.data() + 4 * (size_t)j);
        }
        at += 32 * (size_t)width;
        int32_t open_ok = 0;
        ZKCHK(zk_merkle_verify_host(field, root, m, width, idx[q], limbs.data(), at, &open_ok));
        at += 32 * (size_t)m;
        if (!open_ok) return ZK_OK;
        const uint8_t *r0 = proof + 32 * (R + (1ull << f) + (uint64_t)q * per_query);
        Fe x = fe_mul(s, fe_pow_u64(w, idx[q], P), P);   // x_{idx + j M} = x_idx w_{2^a}^j
        const Fe step = fe_pow_u64(w, 1ull << m, P);
        for (uint32_t j = 0; j < (1u << a); ++j) {
            Fe num = row[((size_t)(k - 1) << a) + j], got;
            for (uint32_t cc = k - 1; cc-- > 0;) num = fe_add(fe_mul(num, alpha, P), row[((size_t)cc << a) + j], P);
            if (!fri_from_be32(r0 + 32 * (size_t)j, P, &got)) return ZK_OK;
            // got (x - z) == x (num - Y), without an inversion (x - z is not zero: z is off the domain)
            if (!fe_eq(fe_mul(got, fe_sub(x, zf, P), P), fe_mul(x, fe_sub(num, y_comb, P), P))) return ZK_OK;
            x = fe_mul(x, step, P);
        }
    }
    *out_ok = 1;
    return ZK_OK;
}

// device time of `reps` quotients of the k columns into `out` between two HIP events after as many untimed ones (the power table and the
// pointer array are made once, outside): shift = the field's generator, z, alpha and Y fixed non-zero elements off the domain
extern "C" int32_t zk_bench_deep_quotient(zk_ctx *c, const zk_mle *const *columns, uint32_t n_columns, zk_mle *out, int32_t reps, double *out_ms) {
    if (!out_ms || reps < 1) return ZK_ERR_BAD_ARG;
    ZKCHK(quotient_columns(c, columns, n_columns, out));
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)out->n_vars;
    if (n > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    ZKCHK(use_device(c));
    const Fe s = fe_from_u32(c->fi->generator, P), z = fe_zero(), alpha = c->fi->two_adic_root, y = fe_from_u32(3, P);   // 0 is on no coset
    std::vector<const uint64_t *> cols;
    try {
        cols.resize(n_columns);
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    for (uint32_t j = 0; j < n_columns; ++j) cols[j] = columns[j]->d;
    PoolScope ps(c);
    QuotientPlan pl;
    DrainOnExit drain(c);   // the plan's kernels: a failed allocation after them waits before the blocks go back
    ZKCHK(quotient_plan(c, ps, cols.data(), n_columns, n, s, &pl));
    auto once = [&] { return quotient_launch(c, pl, n_columns, n, z, y, alpha, out->d); };
    ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
    drain.armed = false;   // the span has waited for ev1
    return ZK_OK;
}
