// fsum.hip -- host side of the fractional-sum (LogUp) argument and of the lookup multiplicities (kernels: fsum_kernels.cuh; the context, table
// handles, prover core and verifier helpers it uses are declared in host_core.hpp).  No reference item; definition: tests/fsum_ref.py;
// DESIGN.md section 18.
//
// N / D = sum_i p[i] / (q[i] + sigma) is proven to a verifier who afterwards needs one evaluation of p and one of q.  The shape is
// gprod.hip's: the prover builds the fraction tree (two heaps: level j at 2^j), then ties level j to level j + 1 with ONE sumcheck of
// degree 3, for j = 1 .. n - 1, all on one transcript kept on the device; the scalar steps between two sumchecks are one-wave kernels
// (k_fsum_chain); the host waits once, for the published block.  Nothing is inverted anywhere.  A layer's polynomial
// E [P0 Q1 + P1 Q0 + lambda Q0 Q1] lists Q0 and Q1 twice, and prove_core folds every table with the term that lists it, so it is
// regrouped as E P0 Q1 + E' S Q0 with S = P1 + lambda Q1 written per layer (k_fsum_comb, lambda read from the device) and E' a second eq
// table: two terms of three tables, the same round polynomials.  The sumchecks fold out of place, so p and q are left intact; with
// sigma != 0 the top level q + sigma is written once, and with p = NULL the top level's constant-one table.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "fsum_kernels.cuh"
#include "prover_state.hpp"

// ZK_FSUM_TREE_FUSE: levels per launch of the tree above the LDS stage, 1 .. kFtreeMaxFuse; 0 = the default (kFtreeFuseDefault)
static uint32_t fsum_tree_fuse() {
    static const uint32_t v = (uint32_t)env_u64("ZK_FSUM_TREE_FUSE", 0, 0, kFtreeMaxFuse);
    return v ? v : kFtreeFuseDefault;
}
enum { kFsumPathDefault = 0, kFsumPathLevels = 1, kFsumPathProof = 2, kFsumPathMult = 3 };

static uint64_t fsum_proof_elems(uint32_t n) { return 2ull * n * n + 2ull * n; }

// NULL = 0; false: not fully reduced
static bool fsum_shift(const uint64_t *shift, const FieldParams &P, Fe *sigma) {
    *sigma = fe_zero();
    return !shift || fri_elem(shift, P, sigma);
}

template <int A>
static void ftree_launch(zk_ctx *c, const uint64_t *src_p, const uint64_t *src_q, uint64_t *heap_p, uint64_t *heap_q, uint32_t m, bool shift,
                         const Fe &sigma) {
    const uint64_t blocks = (1ull << m) / kBlock;   // m >= kFtreeLdsVars: a whole number of workgroups of whole runs
    const uint32_t g = (uint32_t)(blocks < kMaxGridStream ? blocks : kMaxGridStream);
    const FieldParams &P = c->fi->P;
    if (!src_p && shift) k_ftree<A, true, true><<<g, kBlock, 0, c->stream>>>(src_p, src_q, heap_p, heap_q, m, sigma, P);
    else if (!src_p) k_ftree<A, true, false><<<g, kBlock, 0, c->stream>>>(src_p, src_q, heap_p, heap_q, m, sigma, P);
    else if (shift) k_ftree<A, false, true><<<g, kBlock, 0, c->stream>>>(src_p, src_q, heap_p, heap_q, m, sigma, P);
    else k_ftree<A, false, false><<<g, kBlock, 0, c->stream>>>(src_p, src_q, heap_p, heap_q, m, sigma, P);
}
// heap_p, heap_q (2^n elements each) <- the tree over src_p (NULL: all ones), src_q + sigma (2^n elements each, n >= 1), `fuse` levels
// per launch above the LDS stage.  Asynchronous.
static int32_t fsum_tree(zk_ctx *c, const uint64_t *src_p, const uint64_t *src_q, uint32_t n, bool shift, const Fe &sigma, uint32_t fuse,
                         uint64_t *heap_p, uint64_t *heap_q) {
    uint32_t top = n;
    while (top > kFtreeLdsVars) {
        const uint32_t a = fuse < top - kFtreeLdsVars ? fuse : top - kFtreeLdsVars, m = top - a;
        if (a == 2) ftree_launch<2>(c, src_p, src_q, heap_p, heap_q, m, shift, sigma);
        else ftree_launch<1>(c, src_p, src_q, heap_p, heap_q, m, shift, sigma);
        HIPCHK(hipGetLastError());
        src_p = heap_p + 4 * (1ull << m);
        src_q = heap_q + 4 * (1ull << m);
        shift = false;
        top = m;
    }
    k_ftree_lds<<<1, kBlock, 0, c->stream>>>(src_p, src_q, heap_p, heap_q, top, src_p ? 0u : 1u, shift ? 1u : 0u, sigma, c->fi->P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
static_assert(kFtreeMaxFuse == 2, "fsum_tree dispatches the arities 1 and 2");

// p may be NULL (all ones)
static int32_t fsum_table_args(zk_ctx *c, const zk_mle *p, const zk_mle *q) {
    if (q->ctx != c || (p && p->ctx != c)) return ZK_ERR_CONTEXT_MISMATCH;
    if (q->n_vars < 1 || q->n_vars > kMaxVars || (p && p->n_vars != q->n_vars)) return ZK_ERR_BAD_ARG;
    return ZK_OK;
}

extern "C" int32_t zk_mle_fraction_tree(zk_ctx *c, const zk_mle *p, const zk_mle *q, const uint64_t *shift, zk_mle **out_p, zk_mle **out_q) {
    if (!c || !q || !out_p || !out_q) return ZK_ERR_BAD_ARG;
    ZKCHK(fsum_table_args(c, p, q));
    Fe sigma;
    if (!fsum_shift(shift, c->fi->P, &sigma)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    MleHolder hp, hq;
    ZKCHK(mle_alloc(c, q->n_vars, hp.put()));
    ZKCHK(mle_alloc(c, q->n_vars, hq.put()));
    ZKCHK(fsum_tree(c, p ? p->d : nullptr, q->d, (uint32_t)q->n_vars, !fe_is_zero(sigma), sigma, fsum_tree_fuse(), hp->d, hq->d));
    *out_p = hp.release();
    *out_q = hq.release();
    return ZK_OK;
}

extern "C" int32_t zk_fsum_proof_bytes(uint32_t n_vars, uint64_t *out) {
    if (!out || n_vars < 1 || n_vars > kMaxVars) return ZK_ERR_BAD_ARG;
    *out = 32 * fsum_proof_elems(n_vars);
    return ZK_OK;
}

// the transcript's start but for N and D: seed; be64(field id), be64(n), be64(has_p); be32(sigma)
static void fsum_start(Sponge &sp, int32_t field, uint32_t n, bool has_p, const Fe &sigma, const uint8_t seed[32], const FieldParams &P) {
    sp.init();
    sp.update(seed, 32);
    const uint64_t pv[3] = {(uint64_t)field, n, has_p ? 1ull : 0ull};
    uint8_t be[24], eb[32];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 8; ++k) be[8 * i + k] = (uint8_t)(pv[i] >> (8 * (7 - k)));
    sp.update(be, 24);
    fe_to_bytes_be(sigma, P, eb);
    sp.update(eb, 32);
}

// Everything of a proof but its way to the host: the tree, then per layer the two eq tables, S, the sumcheck and the chain step.  The
// proof block [2 n^2 + 2 n proof elements | N | D | r_n | cP_n | cQ_n - sigma] (Montgomery limbs) is left at *d_block; every block comes
// from the caller's scope, which outlives the queued work.  No host wait.
static int32_t fsum_enqueue(zk_ctx *c, const zk_mle *p, const zk_mle *q, const Fe &sigma, const uint8_t seed[32], PoolScope &ps, uint64_t **d_block) {
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)q->n_vars;
    const bool shift = !fe_is_zero(sigma);
    uint64_t *heap_p = nullptr, *heap_q = nullptr, *d_pt[2] = {nullptr, nullptr}, *d_fin = nullptr, *d_state = nullptr, *d_epart = nullptr, *block = nullptr;
    WordSponge *d_sponge = nullptr;
    ZKCHK(ps.get(mle_block_bytes(n), &heap_p));
    ZKCHK(ps.get(mle_block_bytes(n), &heap_q));
    for (int i = 0; i < 2; ++i) ZKCHK(ps.get((size_t)(kMaxVars + 1) * 32, &d_pt[i]));
    ZKCHK(ps.get(kMaxFactors * 32, &d_fin));
    ZKCHK(ps.get(3 * 32, &d_state));   // cP, cQ, lambda
    ZKCHK(ps.get(sizeof(WordSponge), &d_sponge));
    ZKCHK(ps.get(kEpartBlockBytes, &d_epart));
    ZKCHK(ps.get((size_t)(fsum_proof_elems(n) + n + 4) * 32, &block));
    // level n as the top layer's sumcheck reads it: p itself or ones, q itself or q + sigma written once
    const uint64_t *top_p = p ? p->d : nullptr, *top_q = q->d;
    if (!p) {
        uint64_t *ones = nullptr;
        ZKCHK(ps.get(mle_block_bytes(n), &ones));
        k_fsum_ones<<<grid_for(1ull << n), kBlock, 0, c->stream>>>(ones, 1ull << n, P);
        HIPCHK(hipGetLastError());
        top_p = ones;
    }
    if (shift) {
        uint64_t *shifted = nullptr;
        ZKCHK(ps.get(mle_block_bytes(n), &shifted));
        k_fsum_shift<<<grid_for(1ull << n), kBlock, 0, c->stream>>>(q->d, shifted, 1ull << n, sigma, P);
        HIPCHK(hipGetLastError());
        top_q = shifted;
    }
    ZKCHK(fsum_tree(c, p ? p->d : nullptr, q->d, n, shift, sigma, fsum_tree_fuse(), heap_p, heap_q));
    Sponge sp;
    fsum_start(sp, c->field, n, p != nullptr, sigma, seed, P);
    ZKCHK(sponge_to_device(c, sp, d_sponge, d_epart));
    auto level_p = [&](uint32_t j) -> const uint64_t * { return j < n ? heap_p + 4 * (1ull << j) : top_p; };
    auto level_q = [&](uint32_t j) -> const uint64_t * { return j < n ? heap_q + 4 * (1ull << j) : top_q; };
    uint64_t *proof = block, *d_r = d_pt[0], *d_next = d_pt[1];
    // layer 0: (cP_0, cQ_0) = (N, D), the four values are level 1, no sumcheck
    k_fsum_chain<true><<<1, 64, 0, c->stream>>>(d_sponge, level_p(1), level_q(1), heap_p + 4, heap_q + 4, proof, d_next, d_state, P);
    HIPCHK(hipGetLastError());
    proof += 4 * 4;
    std::swap(d_r, d_next);
    const TermSpec ts = {2, {3, 3, 0, 0}};
    for (uint32_t j = 1; j < n; ++j) {
        MleHolder E, E2, S;   // back to the pool at the end of the iteration (stream-ordered reuse)
        ZKCHK(mle_alloc(c, j, E.put()));
        ZKCHK(mle_alloc(c, j, E2.put()));
        ZKCHK(mle_alloc(c, j, S.put()));
        ZKCHK(eq_table_dev(c, d_r, j, E->d));
        ZKCHK(eq_table_dev(c, d_r, j, E2->d));
        const uint64_t h = 1ull << j;
        uint64_t *up_p = const_cast<uint64_t *>(level_p(j + 1)), *up_q = const_cast<uint64_t *>(level_q(j + 1));   // folded out of place: never written
        k_fsum_comb<<<grid_for(h), kBlock, 0, c->stream>>>(up_p + 4 * h, up_q + 4 * h, d_state + 8, S->d, h, P);
        HIPCHK(hipGetLastError());
        zk_mle P0 = {c, j, up_p}, Q0 = {c, j, up_q}, Q1 = {c, j, up_q + 4 * h};
        zk_mle *f[6] = {E.get(), &P0, &Q1, E2.get(), S.get(), &Q0};
        const DeviceChain ch = {d_sponge, proof, d_next + 4, d_fin, d_epart};   // rho lands behind tau's slot: r_{j+1} = (tau, rho)
        ZKCHK(prove_core(c, f, 6, ts, 3, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ch));
        k_fsum_chain<false><<<1, 64, 0, c->stream>>>(d_sponge, d_fin, nullptr, nullptr, nullptr, proof + 4 * (4 * (uint64_t)j), d_next, d_state, P);
        HIPCHK(hipGetLastError());
        proof += 4 * (4 * (uint64_t)j + 4);
        std::swap(d_r, d_next);
    }
    k_fsum_finish<<<1, 64, 0, c->stream>>>(heap_p + 4, heap_q + 4, d_r, d_state, n, sigma, proof, P);
    HIPCHK(hipGetLastError());
    *d_block = block;
    return ZK_OK;
}

extern "C" int32_t zk_fsum_prove(zk_ctx *c, const zk_mle *p, const zk_mle *q, const uint64_t *shift, const uint8_t seed[32], uint64_t out_sum[8],
                                 uint8_t *out_proof, uint64_t *out_point, uint64_t out_claims[8]) {
    if (!c || !q || !seed || !out_sum || !out_proof || !out_point || !out_claims) return ZK_ERR_BAD_ARG;
    ZKCHK(fsum_table_args(c, p, q));
    const FieldParams &P = c->fi->P;
    Fe sigma;
    if (!fsum_shift(shift, P, &sigma)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)q->n_vars;
    const uint64_t pe = fsum_proof_elems(n);
    const size_t bytes = (size_t)(pe + n + 4) * 32;
    // declaration order is the order of the way out: the stream is waited for (drain) before the scratch (ps) goes back
    PoolScope ps(c);
    DrainOnExit drain(c);
    uint64_t *d_block = nullptr;
    uint8_t *stage = nullptr;
    ZKCHK(fsum_enqueue(c, p, q, sigma, seed, ps, &d_block));
    // the one wait of the proof: the block goes to pinned memory by a kernel that also stores the completion word
    ZKCHK(results_staging(c, bytes, &stage));
    const uint32_t seq = next_flag_seq(c);
    ZKCHK(publish_host(c, d_block, reinterpret_cast<uint64_t *>(stage), (uint32_t)(bytes / 8), seq));
    ZKCHK(host_flag_wait(c, seq));
    drain.armed = false;   // the publishing kernel was the stream's last: everything in front of it is done
    const uint64_t *h = reinterpret_cast<const uint64_t *>(stage);
    for (uint64_t i = 0; i < pe; ++i) fe_to_bytes_be(fe_from_u64limbs(h + 4 * i), P, out_proof + 32 * i);
    memcpy(out_sum, h + 4 * pe, 64);
    memcpy(out_point, h + 4 * (pe + 2), (size_t)n * 32);
    memcpy(out_claims, h + 4 * (pe + 2 + n), 64);
    return ZK_OK;
}

// ---- the verifier: host only, no context ---------------------------------------------------------------------------------------------
extern "C" int32_t zk_fsum_verify_host(int32_t field, uint32_t n_vars, int32_t has_p, const uint64_t *shift, const uint8_t seed[32], const uint64_t sum[8],
                                       const uint8_t *proof, uint64_t proof_len, uint64_t *out_point, uint64_t out_claims[8], int32_t *out_ok) {
    if (!seed || !sum || !proof || !out_point || !out_claims || !out_ok) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    const uint32_t n = n_vars;
    uint64_t want_len = 0;
    ZKCHK(zk_fsum_proof_bytes(n, &want_len));
    Fe sigma, N, D;
    if (!fsum_shift(shift, P, &sigma) || !fri_elem(sum, P, &N) || !fri_elem(sum + 4, P, &D) || proof_len != want_len) return ZK_ERR_BAD_ARG;
    std::vector<uint64_t> el;
    try {
        el.resize((size_t)4 * fsum_proof_elems(n));
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    *out_ok = 0;
    if (fe_is_zero(D)) return ZK_OK;   // the product of all denominators: the sum is not defined
    for (uint64_t i = 0; i < fsum_proof_elems(n); ++i) {
        Fe e;
        if (!fri_from_be32(proof + 32 * i, P, &e)) return ZK_OK;   // not canonical: a verdict, not an error
        fe_to_u64limbs(e, el.data() + 4 * i);
    }
    Sponge sp;
    fsum_start(sp, field, n, has_p != 0, sigma, seed, P);
    absorb_elements(sp, sum, 2, P);
    uint64_t r[4 * (kMaxVars + 1)] = {}, rho[4 * (kMaxVars + 1)] = {}, first[4];
    Fe cp = N, cq = D;
    const Fe one = fe_one(P);
    const uint64_t *at = el.data();
    for (uint32_t j = 0; j < n; ++j) {
        Fe claim = fe_zero(), lam = fe_zero();
        if (j >= 1) {
            lam = squeeze_field_element(sp, P);
            fe_to_u64limbs(fe_add(cp, fe_mul(lam, cq, P), P), first);
            if (verify_internal(P, sp, j, 3, first, at, claim, rho) != ZK_OK) return ZK_OK;   // absorbs the combined claim, then the j rounds
            at += 4 * (4 * (size_t)j);
        }
        const Fe p0 = fe_from_u64limbs(at), p1 = fe_from_u64limbs(at + 4), q0 = fe_from_u64limbs(at + 8), q1 = fe_from_u64limbs(at + 12);
        absorb_elements(sp, at, 4, P);
        at += 16;
        const Fe num = fe_add(fe_mul(p0, q1, P), fe_mul(p1, q0, P), P), den = fe_mul(q0, q1, P);
        if (j == 0) {
            if (!fe_eq(N, num) || !fe_eq(D, den)) return ZK_OK;
        } else {
            Fe eq = one;   // eq(r_j, rho)
            for (uint32_t i = 0; i < j; ++i) {
                const Fe x = fe_from_u64limbs(r + 4 * i), y = fe_from_u64limbs(rho + 4 * i), xy = fe_mul(x, y, P);
                eq = fe_mul(eq, fe_sub(fe_add(fe_add(xy, xy, P), one, P), fe_add(x, y, P), P), P);   // (1 - x)(1 - y) + x y
            }
            if (!fe_eq(claim, fe_mul(eq, fe_add(num, fe_mul(lam, den, P), P), P))) return ZK_OK;
        }
        const Fe tau = squeeze_field_element(sp, P);
        fe_to_u64limbs(tau, r);
        memcpy(r + 4, rho, (size_t)j * 32);
        cp = fe_add(p0, fe_mul(tau, fe_sub(p1, p0, P), P), P);
        cq = fe_add(q0, fe_mul(tau, fe_sub(q1, q0, P), P), P);
    }
    if (!has_p && !fe_eq(cp, one)) return ZK_OK;
    memcpy(out_point, r, (size_t)n * 32);
    fe_to_u64limbs(cp, out_claims);
    fe_to_u64limbs(fe_sub(cq, sigma, P), out_claims + 4);
    *out_ok = 1;
    return ZK_OK;
}

// ---- lookup multiplicities ---------------------------------------------------------------------------------------------------------------
static size_t mult_scratch_bytes(uint32_t m) { return ((size_t)3 << m) * 4 + 32; }   // 2^(m+1) slots, 2^m counts, the three counters
// m_out[j] = #{i : witness[i] = table[j]} for the lowest j of each value, from scratch of mult_scratch_bytes(table n): the three counters
// [missing | first_missing | duplicates] are left at *d_counters.  Asynchronous.
static int32_t mult_enqueue(zk_ctx *c, const zk_mle *table, const zk_mle *witness, uint8_t *scratch, uint64_t *m_out, uint64_t **d_counters) {
    const uint32_t m = (uint32_t)table->n_vars;
    const uint64_t rows = 1ull << m, entries = 1ull << witness->n_vars;
    unsigned long long *counters = reinterpret_cast<unsigned long long *>(scratch);
    uint32_t *slots = reinterpret_cast<uint32_t *>(scratch + 32), *counts = slots + 2 * rows;
    HIPCHK(hipMemsetAsync(scratch, 0, mult_scratch_bytes(m), c->stream));
    HIPCHK(hipMemsetAsync(counters + 1, 0xFF, 8, c->stream));   // first_missing: 2^64 - 1 = none
    k_mult_insert<<<grid_for(rows), kBlock, 0, c->stream>>>(table->d, rows, slots, m + 1, counters);
    HIPCHK(hipGetLastError());
    k_mult_count<<<grid_for(entries), kBlock, 0, c->stream>>>(table->d, witness->d, entries, slots, m + 1, counts, counters);
    HIPCHK(hipGetLastError());
    k_mult_finish<<<grid_for(rows), kBlock, 0, c->stream>>>(counts, rows, m_out, c->fi->P);
    HIPCHK(hipGetLastError());
    *d_counters = reinterpret_cast<uint64_t *>(counters);
    return ZK_OK;
}

extern "C" int32_t zk_lookup_multiplicities(zk_ctx *c, const zk_mle *table, const zk_mle *witness, zk_mle **out_m, uint64_t *out_missing,
                                            uint64_t *out_first_missing, uint64_t *out_duplicates) {
    if (!c || !table || !witness || !out_m || !out_missing || !out_first_missing || !out_duplicates) return ZK_ERR_BAD_ARG;
    if (table->ctx != c || witness->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (table->n_vars > kMultMaxTableVars || witness->n_vars > kMultMaxWitnessVars) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    // declaration order is the order of the way out: the stream is waited for (drain) before the scratch goes back
    PoolBlock scratch;
    MleHolder out;
    DrainOnExit drain(c);
    ZKCHK(scratch.alloc(c, mult_scratch_bytes((uint32_t)table->n_vars)));
    ZKCHK(mle_alloc(c, table->n_vars, out.put()));
    uint64_t *d_counters = nullptr;
    uint8_t *stage = nullptr;
    ZKCHK(mult_enqueue(c, table, witness, scratch.as<uint8_t>(), out->d, &d_counters));
    // the one wait: the three counters go to pinned memory by a kernel that also stores the completion word
    ZKCHK(results_staging(c, 32, &stage));
    const uint32_t seq = next_flag_seq(c);
    ZKCHK(publish_host(c, d_counters, reinterpret_cast<uint64_t *>(stage), 3, seq));
    ZKCHK(host_flag_wait(c, seq));
    drain.armed = false;   // the publishing kernel was the stream's last
    const uint64_t *h = reinterpret_cast<const uint64_t *>(stage);
    *out_missing = h[0];
    *out_first_missing = h[1];
    *out_duplicates = h[2];
    *out_m = out.release();
    return ZK_OK;
}

// device time of `reps` runs between two HIP events after as many untimed ones, average ms per run: path 0 = the tree on the default
// route with p = ones (the switch), 1 = the same with one level per launch above the LDS stage, 2 = the whole proof as zk_fsum_prove
// enqueues it (p = ones, no shift, a fixed seed; without the proof block's way to the host and its one wait), 3 = zk_lookup_multiplicities'
// launches with the witness equal to the table q.  q is left intact.
extern "C" int32_t zk_bench_fsum(zk_ctx *c, const zk_mle *q, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !q || !out_ms || reps < 1 || path < 0 || path > 3) return ZK_ERR_BAD_ARG;
    ZKCHK(fsum_table_args(c, nullptr, q));
    if (path == kFsumPathMult && q->n_vars > kMultMaxTableVars) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)q->n_vars;
    const Fe sigma = fe_zero();
    if (path == kFsumPathProof) {
        const uint8_t seed[32] = {};
        DrainOnExit drain(c);
        auto once = [&]() -> int32_t {
            PoolScope ps(c);   // its blocks go back stream-ordered and come out of the pool again on the next call
            uint64_t *d_block = nullptr;
            return fsum_enqueue(c, nullptr, q, sigma, seed, ps, &d_block);
        };
        ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
        drain.armed = false;   // the span has waited for ev1
        return ZK_OK;
    }
    if (path == kFsumPathMult) {
        PoolBlock scratch, m_out;
        DrainOnExit drain(c);
        ZKCHK(scratch.alloc(c, mult_scratch_bytes(n)));
        ZKCHK(m_out.alloc(c, mle_block_bytes(n)));
        auto once = [&]() -> int32_t {
            uint64_t *d_counters = nullptr;
            return mult_enqueue(c, q, q, scratch.as<uint8_t>(), m_out.as(), &d_counters);
        };
        ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
        drain.armed = false;
        return ZK_OK;
    }
    const uint32_t fuse = path == kFsumPathDefault ? fsum_tree_fuse() : 1;
    PoolBlock heap_p, heap_q;
    DrainOnExit drain(c);
    ZKCHK(heap_p.alloc(c, mle_block_bytes(n)));
    ZKCHK(heap_q.alloc(c, mle_block_bytes(n)));
    auto once = [&]() -> int32_t { return fsum_tree(c, nullptr, q->d, n, false, sigma, fuse, heap_p.as(), heap_q.as()); };
    ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
    drain.armed = false;
    return ZK_OK;
}
