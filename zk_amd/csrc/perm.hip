// perm.hip -- host side of the wiring (copy-constraint) permutation argument (kernels: perm_kernels.cuh; the grand product's tree and layers it
// runs on are gprod.hip's, declared in host_core.hpp).  No reference item; definition: tests/perm_ref.py; DESIGN.md section 21.
//
// k witness columns w_c and k permutation columns sigma_c of n variables satisfy w(sigma(cell)) = w(cell) iff the two sides of the
// fingerprint table F (perm_kernels.cuh) have the same product.  The proof is the grand-product proof of F -- made on the device, never
// uploaded -- whose layer 0 shows the two side products a, b, and the 2 k values of the columns at the low part of its point: the
// verifier is left with 2 k claims at ONE point.  The default route writes F (k_perm_leaves) and runs gprod_tree over it; the other one
// (ZK_PERM_FUSE=1) writes F and the first levels of the tree in one launch (k_perm_tree<A>) and measures slower (profiles/perm.log); both
// make the same bytes.  Two host waits: the
// grand product's block (its point picks the end values' point), then the 2 k values.  The columns are left intact.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "perm_kernels.cuh"

// ZK_PERM_FUSE: 0 = a leaves-only launch, then the tree over F (the default: it measures faster, profiles/perm.log), 1 = F and the tree's
// first launch in one kernel
static bool perm_fuse() {
    static const bool v = env_u64("ZK_PERM_FUSE", 0, 0, 1) != 0;
    return v;
}
// ZK_PERM_MAX_GRID: the cap of k_perm_tree's grid (a wave loops over its runs above it): a small value sends a small shape round the loop
static uint32_t perm_max_grid() {
    static const uint32_t v = (uint32_t)env_u64("ZK_PERM_MAX_GRID", kMaxGridStream, 1, kMaxGridStream);
    return v;
}
enum { kPermPathDefault = 0, kPermPathUnfused = 1, kPermPathProof = 2, kPermPathFused = 3 };

static uint32_t perm_kappa(uint32_t k) {
    uint32_t kp = 0;
    while ((1u << kp) < k) ++kp;
    return kp;
}
static uint64_t perm_head_elems(uint32_t N) { return 2ull * N * N; }

// the shapes of a statement: k in 1 .. 16, n >= 1, N = n + kappa + 1 <= 40
static bool perm_shape(uint64_t n, uint32_t k, uint32_t *N) {
    if (k < 1 || k > kPermMaxCols || n < 1 || n > kMaxVars) return false;
    *N = (uint32_t)n + perm_kappa(k) + 1;
    return *N <= kMaxVars;
}
extern "C" int32_t zk_perm_proof_bytes(uint32_t n_vars, uint32_t k, uint64_t *out) {
    uint32_t N = 0;
    if (!out || !perm_shape(n_vars, k, &N)) return ZK_ERR_BAD_ARG;
    *out = 32 * (perm_head_elems(N) + 2 * k);
    return ZK_OK;
}

// every table non-NULL, of this context, of one n_vars; the shape (the caller has checked c, w and sigma)
static int32_t perm_table_args(zk_ctx *c, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, uint32_t *N) {
    const uint32_t kk = k < kPermMaxCols ? k : kPermMaxCols;   // what a caller with a bad k has at least
    for (uint32_t i = 0; i < kk; ++i)
        if (!w[i] || !sigma[i]) return ZK_ERR_BAD_ARG;
    for (uint32_t i = 0; i < kk; ++i)
        if (w[i]->ctx != c || sigma[i]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (k < 1 || k > kPermMaxCols) return ZK_ERR_BAD_ARG;
    for (uint32_t i = 0; i < k; ++i)
        if (w[i]->n_vars != w[0]->n_vars || sigma[i]->n_vars != w[0]->n_vars) return ZK_ERR_BAD_ARG;
    return perm_shape(w[0]->n_vars, k, N) ? ZK_OK : ZK_ERR_BAD_ARG;
}

// seed' = Keccak-256(seed | be64(field id) be64(n) be64(k) | be32(beta) | be32(gamma)): the grand product's seed
static void perm_seed(int32_t field, uint32_t n, uint32_t k, const Fe &beta, const Fe &gamma, const uint8_t seed[32], const FieldParams &P,
                      uint8_t out[32]) {
    Sponge sp;
    sp.init();
    sp.update(seed, 32);
    const uint64_t pv[3] = {(uint64_t)field, n, k};
    uint8_t be[24], eb[32];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 8; ++j) be[8 * i + j] = (uint8_t)(pv[i] >> (8 * (7 - j)));
    sp.update(be, 24);
    fe_to_bytes_be(beta, P, eb);
    sp.update(eb, 32);
    fe_to_bytes_be(gamma, P, eb);
    sp.update(eb, 32);
    sp.finalize_reset(out);
}
static Fe perm_fe_u64(uint64_t v, const FieldParams &P) {
    const Fe raw = {{(uint32_t)v, (uint32_t)(v >> 32), 0, 0, 0, 0, 0, 0}};
    return fe_from_canonical(raw, P);
}

// ---- the device side ---------------------------------------------------------------------------------------------------------------
struct PermSide {
    PermArgs a = {};
    uint32_t n = 0, k = 0, N = 0;
    Fe beta;
    // the pointer table (a block of the caller's scope, written by a launch: no staging, no wait) and the kernels' constants
    int32_t init(zk_ctx *c, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t kk, uint32_t NN, const Fe &b, const Fe &gamma, PoolScope &ps) {
        const FieldParams &P = c->fi->P;
        n = (uint32_t)w[0]->n_vars, k = kk, N = NN, beta = b;
        const uint64_t **d_cols = nullptr;
        ZKCHK(ps.get(sizeof(PermCols), &d_cols));
        PermCols pc = {};
        for (uint32_t i = 0; i < k; ++i) pc.p[i] = w[i]->d, pc.p[k + i] = sigma[i]->d;
        k_perm_cols<<<1, 64, 0, c->stream>>>(pc, d_cols);
        HIPCHK(hipGetLastError());
        a.cols = d_cols;
        a.n = n, a.k = k;
        a.gamma = gamma, a.one = fe_one(P);
        a.beta_rr = fe_from_canonical(beta, P);
        a.beta29 = mul29_prepare(beta, P);
        return ZK_OK;
    }
    // F (2^N elements) alone
    int32_t leaves(zk_ctx *c, uint64_t *F) const {
        const uint64_t cells = 1ull << (N - 1);
        k_perm_leaves<<<grid_for(cells), kBlock, 0, c->stream>>>(a, cells, F, c->fi->P);
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    // F and the whole heap of its tree (2^N elements each).  fused: F and the first A levels in one launch where the tree has a launch
    // above the LDS stage (N > gprod_lds_vars(), so n >= 6), A as gprod_tree would take it but at most kPermMaxFuse
    int32_t build(zk_ctx *c, bool fused, uint32_t fuse, uint64_t *F, uint64_t *heap) const {
        const FieldParams &P = c->fi->P;
        const uint32_t lds = gprod_lds_vars();
        if (!fused || N <= lds || n < 6) {
            ZKCHK(leaves(c, F));
            return gprod_tree(c, F, N, false, fe_zero(), fuse, heap);
        }
        const uint32_t want = fuse < kPermMaxFuse ? fuse : kPermMaxFuse, A = want < N - lds ? want : N - lds, m = N - A - 1;
        PermArgs b = a;
        b.beta_stride = fe_mul(beta, perm_fe_u64(1ull << m, P), P);
        const uint64_t blocks = (1ull << m) / kBlock;   // m >= gprod_lds_vars() - 1: a whole number of workgroups of whole runs
        const uint32_t cap = perm_max_grid(), g = (uint32_t)(blocks < cap ? blocks : cap);
        if (A == 2) k_perm_tree<2><<<g, kBlock, 0, c->stream>>>(b, m, F, heap, P);
        else k_perm_tree<1><<<g, kBlock, 0, c->stream>>>(b, m, F, heap, P);
        HIPCHK(hipGetLastError());
        return gprod_tree(c, heap + 4 * (1ull << (N - A)), N - A, false, fe_zero(), fuse, heap);
    }
};

extern "C" int32_t zk_mle_perm_fingerprint(zk_ctx *c, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, const uint64_t beta[4],
                                           const uint64_t gamma[4], zk_mle **out) {
    if (!c || !w || !sigma || !beta || !gamma || !out) return ZK_ERR_BAD_ARG;
    uint32_t N = 0;
    ZKCHK(perm_table_args(c, w, sigma, k, &N));
    const FieldParams &P = c->fi->P;
    Fe b, g;
    if (!fri_elem(beta, P, &b) || !fri_elem(gamma, P, &g)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    PoolScope ps(c);
    MleHolder F;
    ZKCHK(mle_alloc(c, N, F.put()));
    PermSide side;
    ZKCHK(side.init(c, w, sigma, k, N, b, g, ps));
    ZKCHK(side.leaves(c, F->d));
    *out = F.release();
    return ZK_OK;
}

// Everything of a proof but its way to the host and its end values: the pointer table, F, the tree, the grand product's layers under
// seed'.  The grand product's block is left at s->block; every block comes from the caller's scope.  No host wait.
static int32_t perm_enqueue(zk_ctx *c, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, uint32_t N, const Fe &beta, const Fe &gamma,
                            const uint8_t seed[32], bool fused, PoolScope &ps, GprodScratch *s) {
    uint64_t *F = nullptr;
    ZKCHK(gprod_scratch(ps, N, s));
    ZKCHK(ps.get(mle_block_bytes(N), &F));
    PermSide side;
    ZKCHK(side.init(c, w, sigma, k, N, beta, gamma, ps));
    ZKCHK(side.build(c, fused, gprod_tree_fuse(), F, s->heap));
    uint8_t seed2[32];
    perm_seed(c->field, side.n, k, beta, gamma, seed, c->fi->P, seed2);
    return gprod_layers(c, N, F, *s, fe_zero(), seed2);
}
// the 2 k end values w_c(point), sigma_c(point) into d_vals, by zk_mle_evaluate's launches
static int32_t perm_end_values(zk_ctx *c, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, const uint64_t *point, uint64_t *d_vals) {
    for (uint32_t i = 0; i < 2 * k; ++i) ZKCHK(evaluate_device(c, i < k ? w[i] : sigma[i - k], point, d_vals + 4 * i));
    return ZK_OK;
}

extern "C" int32_t zk_perm_prove(zk_ctx *c, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, const uint64_t beta[4],
                                 const uint64_t gamma[4], const uint8_t seed[32], uint8_t *out_proof, uint64_t *out_point, uint64_t *out_claims) {
    if (!c || !w || !sigma || !beta || !gamma || !seed || !out_proof || !out_point || !out_claims) return ZK_ERR_BAD_ARG;
    uint32_t N = 0;
    ZKCHK(perm_table_args(c, w, sigma, k, &N));
    const FieldParams &P = c->fi->P;
    Fe b, g;
    if (!fri_elem(beta, P, &b) || !fri_elem(gamma, P, &g)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)w[0]->n_vars, kp = perm_kappa(k);
    const uint64_t pe = perm_head_elems(N);
    const size_t bytes = (size_t)(pe + N + 2) * 32;
    // declaration order is the order of the way out: the stream is waited for (drain) before the scratch (ps) goes back
    PoolScope ps(c);
    DrainOnExit drain(c);
    GprodScratch s;
    uint64_t *d_vals = nullptr;
    uint8_t *stage = nullptr;
    std::vector<uint64_t> head;
    try {
        head.resize(4 * (pe + N));
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    ZKCHK(ps.get((size_t)2 * kPermMaxCols * 32, &d_vals));
    ZKCHK(perm_enqueue(c, w, sigma, k, N, b, g, seed, perm_fuse(), ps, &s));
    // the first wait: the grand product's block, whose point picks the point of the end values
    ZKCHK(results_staging(c, bytes, &stage));
    const uint32_t seq = next_flag_seq(c);
    ZKCHK(publish_host(c, s.block, reinterpret_cast<uint64_t *>(stage), (uint32_t)(bytes / 8), seq));
    ZKCHK(host_flag_wait(c, seq));
    const uint64_t *h = reinterpret_cast<const uint64_t *>(stage);
    memcpy(head.data(), h, (size_t)pe * 32);
    memcpy(head.data() + 4 * pe, h + 4 * (pe + 1), (size_t)N * 32);   // r_N behind the product
    const uint64_t *r_lo = head.data() + 4 * (pe + kp);
    // the second wait: the 2 k values at r_lo
    ZKCHK(perm_end_values(c, w, sigma, k, r_lo, d_vals));
    HIPCHK(hipMemcpyAsync(c->h_pinned, d_vals, (size_t)2 * k * 32, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    for (uint64_t i = 0; i < pe; ++i) fe_to_bytes_be(fe_from_u64limbs(head.data() + 4 * i), P, out_proof + 32 * i);
    for (uint32_t i = 0; i < 2 * k; ++i) fe_to_bytes_be(fe_from_u64limbs(c->h_pinned + 4 * i), P, out_proof + 32 * (pe + i));
    memcpy(out_point, r_lo, (size_t)n * 32);
    memcpy(out_claims, c->h_pinned, (size_t)2 * k * 32);
    return ZK_OK;
}

// ---- the verifier: host only, no context; nothing sized by 2^n ----------------------------------------------------------------------
extern "C" int32_t zk_perm_verify_host(int32_t field, uint32_t n_vars, uint32_t k, const uint64_t beta[4], const uint64_t gamma[4],
                                       const uint8_t seed[32], const uint8_t *proof, uint64_t proof_len, uint64_t *out_point, uint64_t *out_claims,
                                       int32_t *out_ok) {
    if (!beta || !gamma || !seed || !proof || !out_point || !out_claims || !out_ok) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    uint64_t want_len = 0;
    ZKCHK(zk_perm_proof_bytes(n_vars, k, &want_len));
    Fe b, g;
    if (!fri_elem(beta, P, &b) || !fri_elem(gamma, P, &g) || proof_len != want_len) return ZK_ERR_BAD_ARG;
    const uint32_t n = n_vars, kp = perm_kappa(k), N = n + kp + 1;
    const uint64_t pe = perm_head_elems(N);
    Fe vals[2 * kPermMaxCols], pa, pb;
    for (uint32_t i = 0; i < 2 * k; ++i)
        if (!fri_from_be32(proof + 32 * (pe + i), P, &vals[i])) {   // not canonical: a verdict, not an error
            *out_ok = 0;
            return ZK_OK;
        }
    if (!fri_from_be32(proof, P, &pa) || !fri_from_be32(proof + 32, P, &pb) || !fe_eq(pa, pb)) {
        *out_ok = 0;
        return ZK_OK;
    }
    uint8_t seed2[32];
    perm_seed(field, n, k, b, g, seed, P, seed2);
    uint64_t product[4], r[4 * (kMaxVars + 1)], claim_l[4];
    fe_to_u64limbs(fe_mul(pa, pb, P), product);
    int32_t ok = 0;
    ZKCHK(zk_gprod_verify_host(field, N, nullptr, seed2, product, proof, 32 * pe, r, claim_l, &ok));
    *out_ok = 0;
    if (!ok) return ZK_OK;
    const Fe one = fe_one(P), r_s = fe_from_u64limbs(r + 4 * (kp + n)), not_s = fe_sub(one, r_s, P);
    Fe ident = fe_zero();   // sum_b r_lo[b] 2^(n-1-b)
    for (uint32_t j = 0; j < n; ++j) ident = fe_add(fe_add(ident, ident, P), fe_from_u64limbs(r + 4 * (kp + j)), P);
    Fe total = fe_zero();
    for (uint32_t col = 0; col < (1u << kp); ++col) {
        Fe eq = one;   // eq(r_hi, col): variable 0 = the top bit
        for (uint32_t j = 0; j < kp; ++j) {
            const Fe x = fe_from_u64limbs(r + 4 * j);
            eq = fe_mul(eq, ((col >> (kp - 1 - j)) & 1) ? x : fe_sub(one, x, P), P);
        }
        Fe term = one;
        if (col < k) {
            const Fe label = fe_add(fe_mul(not_s, fe_add(perm_fe_u64((uint64_t)col << n, P), ident, P), P), fe_mul(r_s, vals[k + col], P), P);
            term = fe_add(fe_add(vals[col], fe_mul(b, label, P), P), g, P);
        }
        total = fe_add(total, fe_mul(eq, term, P), P);
    }
    if (!fe_eq(total, fe_from_u64limbs(claim_l))) return ZK_OK;
    memcpy(out_point, r + 4 * kp, (size_t)n * 32);
    for (uint32_t i = 0; i < 2 * k; ++i) fe_to_u64limbs(vals[i], out_claims + 4 * i);
    *out_ok = 1;
    return ZK_OK;
}

// device time of `reps` runs between two HIP events after as many untimed ones, average ms per run: path 0 = F and its tree on the default
// route (the switches), 1 = the same on the unfused route, 3 = on the fused route, 2 = the whole proof as zk_perm_prove enqueues it (beta =
// 2, gamma = 1, a fixed seed; the 2 k evaluations at a fixed point; without the two ways to the host and their waits).  The columns are
// left intact.
extern "C" int32_t zk_bench_perm(zk_ctx *c, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !w || !sigma || !out_ms || reps < 1 || path < 0 || path > 3) return ZK_ERR_BAD_ARG;
    uint32_t N = 0;
    ZKCHK(perm_table_args(c, w, sigma, k, &N));
    ZKCHK(use_device(c));
    const FieldParams &P = c->fi->P;
    const Fe gamma = fe_one(P), beta = fe_add(gamma, gamma, P);
    if (path == kPermPathProof) {
        const uint8_t seed[32] = {};
        uint64_t point[4 * kMaxVars];
        for (uint32_t j = 0; j < (uint32_t)w[0]->n_vars; ++j) fe_to_u64limbs(beta, point + 4 * j);
        DrainOnExit drain(c);
        auto once = [&]() -> int32_t {
            PoolScope ps(c);   // its blocks go back stream-ordered and come out of the pool again on the next call
            GprodScratch s;
            uint64_t *d_vals = nullptr;
            ZKCHK(ps.get((size_t)2 * kPermMaxCols * 32, &d_vals));
            ZKCHK(perm_enqueue(c, w, sigma, k, N, beta, gamma, seed, perm_fuse(), ps, &s));
            return perm_end_values(c, w, sigma, k, point, d_vals);
        };
        ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
        drain.armed = false;   // the span has waited for ev1
        return ZK_OK;
    }
    PoolScope ps(c);
    DrainOnExit drain(c);
    uint64_t *F = nullptr, *heap = nullptr;
    ZKCHK(ps.get(mle_block_bytes(N), &F));
    ZKCHK(ps.get(mle_block_bytes(N), &heap));
    PermSide side;
    ZKCHK(side.init(c, w, sigma, k, N, beta, gamma, ps));
    const bool fused = path == kPermPathFused || (path == kPermPathDefault && perm_fuse());
    auto once = [&]() -> int32_t { return side.build(c, fused, gprod_tree_fuse(), F, heap); };
    ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
    drain.armed = false;
    return ZK_OK;
}
