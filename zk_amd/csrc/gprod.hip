// gprod.hip -- host side of the grand-product argument (kernels: gprod_kernels.cuh; the context, table handles, prover core and verifier
// helpers it uses are declared in host_core.hpp).  No reference item; definition: tests/gprod_ref.py; DESIGN.md section 17.
//
// P = prod_i (t[i] + sigma) is proven to a verifier who afterwards needs one evaluation of t.  The prover builds the product tree (a heap:
// level j at 2^j), then ties level j to level j + 1 with ONE sumcheck of degree 3 over E = eq(., r_j), A, B = the two halves of level j + 1
// (prove_core in DeviceChain mode, as it stands), for j = 1 .. n - 1; layer 0 needs none.  The whole proof runs on one transcript kept on
// the device: the eq table of r_j is built from the device-resident point, the scalar steps between two sumchecks are one-wave kernels
// (k_gprod_chain), the round polynomials land in the device proof block, and the host waits once, for the published block.  The tree's
// levels are views into the heap (zk_mle values on the stack, never handed out); the sumchecks fold them out of place, so the table t --
// the top level when sigma = 0 -- is left intact; with sigma != 0 the top level t + sigma is written once for its sumcheck.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "gprod_kernels.cuh"
#include "prover_state.hpp"

// ZK_GPROD_TREE_FUSE: levels per launch of the tree above the LDS stage, 1 .. 3; 0 = the default (kPtreeFuseDefault, tools/gprod_bench.py)
uint32_t zk::gprod_tree_fuse() {
    static const uint32_t v = (uint32_t)env_u64("ZK_GPROD_TREE_FUSE", 0, 0, kPtreeMaxFuse);
    return v ? v : kPtreeFuseDefault;
}
uint32_t zk::gprod_lds_vars() { return kPtreeLdsVars; }
enum { kGprodPathDefault = 0, kGprodPathLevels = 1, kGprodPathProof = 2 };

static uint64_t gprod_proof_elems(uint32_t n) { return 2ull * n * n; }

// NULL = 0; false: not fully reduced
static bool gprod_shift(const uint64_t *shift, const FieldParams &P, Fe *sigma) {
    *sigma = fe_zero();
    return !shift || fri_elem(shift, P, sigma);
}

template <int A>
static void ptree_launch(zk_ctx *c, const uint64_t *src, uint64_t *heap, uint32_t m, bool shift, const Fe &sigma) {
    const uint64_t blocks = (1ull << m) / kBlock;   // m >= kPtreeLdsVars: a whole number of workgroups of whole runs
    const uint32_t g = (uint32_t)(blocks < kMaxGridStream ? blocks : kMaxGridStream);
    if (shift) k_ptree<A, true><<<g, kBlock, 0, c->stream>>>(src, heap, m, sigma, c->fi->P);
    else k_ptree<A, false><<<g, kBlock, 0, c->stream>>>(src, heap, m, sigma, c->fi->P);
}
// heap (2^n elements) <- the tree over src + sigma (2^n elements, n >= 1), `fuse` levels per launch above the LDS stage.  Asynchronous.
int32_t zk::gprod_tree(zk_ctx *c, const uint64_t *src, uint32_t n, bool shift, const Fe &sigma, uint32_t fuse, uint64_t *heap) {
    uint32_t top = n;
    while (top > kPtreeLdsVars) {
        const uint32_t a = fuse < top - kPtreeLdsVars ? fuse : top - kPtreeLdsVars, m = top - a;
        if (a == 3) ptree_launch<3>(c, src, heap, m, shift, sigma);
        else if (a == 2) ptree_launch<2>(c, src, heap, m, shift, sigma);
        else ptree_launch<1>(c, src, heap, m, shift, sigma);
        HIPCHK(hipGetLastError());
        src = heap + 4 * (1ull << m);
        shift = false;
        top = m;
    }
    k_ptree_lds<<<1, kBlock, 0, c->stream>>>(src, heap, top, shift ? 1u : 0u, sigma, c->fi->P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

static int32_t gprod_table_args(zk_ctx *c, const zk_mle *t) {
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (t->n_vars < 1 || t->n_vars > kMaxVars) return ZK_ERR_BAD_ARG;
    return ZK_OK;
}

extern "C" int32_t zk_mle_product_tree(zk_ctx *c, const zk_mle *t, const uint64_t *shift, zk_mle **out) {
    if (!c || !t || !out) return ZK_ERR_BAD_ARG;
    ZKCHK(gprod_table_args(c, t));
    Fe sigma;
    if (!gprod_shift(shift, c->fi->P, &sigma)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    MleHolder heap;
    ZKCHK(mle_alloc(c, t->n_vars, heap.put()));
    ZKCHK(gprod_tree(c, t->d, (uint32_t)t->n_vars, !fe_is_zero(sigma), sigma, gprod_tree_fuse(), heap->d));
    *out = heap.release();
    return ZK_OK;
}

extern "C" int32_t zk_gprod_proof_bytes(uint32_t n_vars, uint64_t *out) {
    if (!out || n_vars < 1 || n_vars > kMaxVars) return ZK_ERR_BAD_ARG;
    *out = 32 * gprod_proof_elems(n_vars);
    return ZK_OK;
}

// the transcript's start: seed; be64(field id), be64(n); be32(sigma)
static void gprod_start(Sponge &sp, int32_t field, uint32_t n, const Fe &sigma, const uint8_t seed[32], const FieldParams &P) {
    sp.init();
    sp.update(seed, 32);
    const uint64_t pv[2] = {(uint64_t)field, n};
    uint8_t be[16], eb[32];
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 8; ++k) be[8 * i + k] = (uint8_t)(pv[i] >> (8 * (7 - k)));
    sp.update(be, 16);
    fe_to_bytes_be(sigma, P, eb);
    sp.update(eb, 32);
}

// The scratch of a proof's layers, from the caller's scope (which outlives the queued work): the heap and the transcript's blocks
int32_t zk::gprod_scratch(PoolScope &ps, uint32_t n, GprodScratch *s) {
    ZKCHK(ps.get(mle_block_bytes(n), &s->heap));
    for (int i = 0; i < 2; ++i) ZKCHK(ps.get((size_t)(kMaxVars + 1) * 32, &s->d_pt[i]));
    ZKCHK(ps.get(kMaxFactors * 32, &s->d_fin));
    ZKCHK(ps.get(32, &s->d_claim));
    ZKCHK(ps.get(sizeof(WordSponge), &s->d_sponge));
    ZKCHK(ps.get(kEpartBlockBytes, &s->d_epart));
    ZKCHK(ps.get((size_t)(gprod_proof_elems(n) + n + 2) * 32, &s->block));
    return ZK_OK;
}
// The layers of a proof on a tree that is already queued: s.heap holds levels n - 1 .. 0 of the tree over `top` (level n as the top
// layer's sumcheck reads it, t + sigma).  Per layer the eq table, the sumcheck and the chain step; the proof block [2 n^2 proof elements |
// P | r_n | c_n - sigma] (Montgomery limbs) is left at s.block.  No host wait.
int32_t zk::gprod_layers(zk_ctx *c, uint32_t n, const uint64_t *top, const GprodScratch &s, const Fe &sigma, const uint8_t seed[32]) {
    const FieldParams &P = c->fi->P;
    uint64_t *heap = s.heap, *d_fin = s.d_fin, *d_claim = s.d_claim, *d_epart = s.d_epart;
    WordSponge *d_sponge = s.d_sponge;
    Sponge sp;
    gprod_start(sp, c->field, n, sigma, seed, P);
    ZKCHK(sponge_to_device(c, sp, d_sponge, d_epart));
    auto level = [&](uint32_t j) -> const uint64_t * { return j < n ? heap + 4 * (1ull << j) : top; };
    uint64_t *proof = s.block, *d_r = s.d_pt[0], *d_next = s.d_pt[1];
    // layer 0: c_0 = P, a = V_1[0], b = V_1[1], no sumcheck
    k_gprod_chain<true><<<1, 64, 0, c->stream>>>(d_sponge, heap + 4, level(1), proof, d_next, d_claim, P);
    HIPCHK(hipGetLastError());
    proof += 4 * 2;
    std::swap(d_r, d_next);
    const TermSpec ts = {1, {3, 0, 0, 0}};
    for (uint32_t j = 1; j < n; ++j) {
        MleHolder E;   // back to the pool at the end of the iteration (stream-ordered reuse)
        ZKCHK(mle_alloc(c, j, E.put()));
        ZKCHK(eq_table_dev(c, d_r, j, E->d));
        uint64_t *up = const_cast<uint64_t *>(level(j + 1));   // folded out of place (consume = 0): never written
        zk_mle A = {c, j, up}, B = {c, j, up + 4 * (1ull << j)};
        zk_mle *f[3] = {E.get(), &A, &B};
        const DeviceChain ch = {d_sponge, proof, d_next + 4, d_fin, d_epart};   // rho lands behind tau's slot: r_{j+1} = (tau, rho)
        ZKCHK(prove_core(c, f, 3, ts, 3, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ch));
        k_gprod_chain<false><<<1, 64, 0, c->stream>>>(d_sponge, nullptr, d_fin + 4, proof + 4 * (4 * (uint64_t)j), d_next, d_claim, P);
        HIPCHK(hipGetLastError());
        proof += 4 * (4 * (uint64_t)j + 2);
        std::swap(d_r, d_next);
    }
    k_gprod_finish<<<1, 64, 0, c->stream>>>(heap + 4, d_r, d_claim, n, sigma, proof, P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// Everything of a proof but its way to the host: the tree, then the layers.  The proof block is left at *d_block; every block comes from
// the caller's scope, which outlives the queued work.  No host wait.
static int32_t gprod_enqueue(zk_ctx *c, const zk_mle *t, const Fe &sigma, const uint8_t seed[32], PoolScope &ps, uint64_t **d_block) {
    const FieldParams &P = c->fi->P;
    const uint32_t n = (uint32_t)t->n_vars;
    const bool shift = !fe_is_zero(sigma);
    GprodScratch s;
    ZKCHK(gprod_scratch(ps, n, &s));
    // level n as the top layer's sumcheck reads it: t itself, or t + sigma written once
    const uint64_t *top = t->d;
    if (shift) {
        uint64_t *shifted = nullptr;
        ZKCHK(ps.get(mle_block_bytes(n), &shifted));
        k_gprod_shift<<<grid_for(1ull << n), kBlock, 0, c->stream>>>(t->d, shifted, 1ull << n, sigma, P);
        HIPCHK(hipGetLastError());
        top = shifted;
    }
    ZKCHK(gprod_tree(c, t->d, n, shift, sigma, gprod_tree_fuse(), s.heap));
    ZKCHK(gprod_layers(c, n, top, s, sigma, seed));
    *d_block = s.block;
    return ZK_OK;
}

extern "C" int32_t zk_gprod_prove(zk_ctx *c, const zk_mle *t, const uint64_t *shift, const uint8_t seed[32], uint64_t out_product[4],
                                  uint8_t *out_proof, uint64_t *out_point, uint64_t out_claim[4]) {
    if (!c || !t || !seed || !out_product || !out_proof || !out_point || !out_claim) return ZK_ERR_BAD_ARG;
    ZKCHK(gprod_table_args(c, t));
    const FieldParams &P = c->fi->P;
    Fe sigma;
    if (!gprod_shift(shift, P, &sigma)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)t->n_vars;
    const uint64_t pe = gprod_proof_elems(n);
    const size_t bytes = (size_t)(pe + n + 2) * 32;
    // declaration order is the order of the way out: the stream is waited for (drain) before the scratch (ps) goes back
    PoolScope ps(c);
    DrainOnExit drain(c);
    uint64_t *d_block = nullptr;
    uint8_t *stage = nullptr;
    ZKCHK(gprod_enqueue(c, t, sigma, seed, ps, &d_block));
    // the one wait of the proof: the block goes to pinned memory by a kernel that also stores the completion word
    ZKCHK(results_staging(c, bytes, &stage));
    const uint32_t seq = next_flag_seq(c);
    ZKCHK(publish_host(c, d_block, reinterpret_cast<uint64_t *>(stage), (uint32_t)(bytes / 8), seq));
    ZKCHK(host_flag_wait(c, seq));
    drain.armed = false;   // the publishing kernel was the stream's last: everything in front of it is done
    const uint64_t *h = reinterpret_cast<const uint64_t *>(stage);
    for (uint64_t i = 0; i < pe; ++i) fe_to_bytes_be(fe_from_u64limbs(h + 4 * i), P, out_proof + 32 * i);
    memcpy(out_product, h + 4 * pe, 32);
    memcpy(out_point, h + 4 * (pe + 1), (size_t)n * 32);
    memcpy(out_claim, h + 4 * (pe + 1 + n), 32);
    return ZK_OK;
}

// ---- the verifier: host only, no context ---------------------------------------------------------------------------------------------
extern "C" int32_t zk_gprod_verify_host(int32_t field, uint32_t n_vars, const uint64_t *shift, const uint8_t seed[32], const uint64_t product[4],
                                        const uint8_t *proof, uint64_t proof_len, uint64_t *out_point, uint64_t out_claim[4], int32_t *out_ok) {
    if (!seed || !product || !proof || !out_point || !out_claim || !out_ok) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    const FieldParams &P = fi->P;
    const uint32_t n = n_vars;
    uint64_t want_len = 0;
    ZKCHK(zk_gprod_proof_bytes(n, &want_len));
    Fe sigma, prod;
    if (!gprod_shift(shift, P, &sigma) || !fri_elem(product, P, &prod) || proof_len != want_len) return ZK_ERR_BAD_ARG;
    std::vector<uint64_t> el;
    try {
        el.resize((size_t)4 * gprod_proof_elems(n));
    } catch (...) {
        return ZK_ERR_ALLOC;
    }
    *out_ok = 0;
    for (uint64_t i = 0; i < gprod_proof_elems(n); ++i) {
        Fe e;
        if (!fri_from_be32(proof + 32 * i, P, &e)) return ZK_OK;   // not canonical: a verdict, not an error
        fe_to_u64limbs(e, el.data() + 4 * i);
    }
    Sponge sp;
    gprod_start(sp, field, n, sigma, seed, P);
    uint64_t r[4 * (kMaxVars + 1)] = {}, rho[4 * (kMaxVars + 1)] = {}, sum[4];
    Fe c = prod;
    const Fe one = fe_one(P);
    const uint64_t *at = el.data();
    for (uint32_t j = 0; j < n; ++j) {
        fe_to_u64limbs(c, sum);
        Fe claim;
        if (verify_internal(P, sp, j, 3, sum, at, claim, rho) != ZK_OK) return ZK_OK;   // absorbs c_j, then the j rounds
        at += 4 * (4 * (size_t)j);
        const Fe a = fe_from_u64limbs(at), b = fe_from_u64limbs(at + 4);
        absorb_elements(sp, at, 2, P);
        at += 8;
        Fe eq = one;   // eq(r_j, rho)
        for (uint32_t i = 0; i < j; ++i) {
            const Fe x = fe_from_u64limbs(r + 4 * i), y = fe_from_u64limbs(rho + 4 * i), xy = fe_mul(x, y, P);
            eq = fe_mul(eq, fe_sub(fe_add(fe_add(xy, xy, P), one, P), fe_add(x, y, P), P), P);   // (1 - x)(1 - y) + x y
        }
        if (!fe_eq(claim, fe_mul(eq, fe_mul(a, b, P), P))) return ZK_OK;
        const Fe tau = squeeze_field_element(sp, P);
        fe_to_u64limbs(tau, r);
        memcpy(r + 4, rho, (size_t)j * 32);
        c = fe_add(a, fe_mul(tau, fe_sub(b, a, P), P), P);
    }
    memcpy(out_point, r, (size_t)n * 32);
    fe_to_u64limbs(fe_sub(c, sigma, P), out_claim);
    *out_ok = 1;
    return ZK_OK;
}

// device time of `reps` runs between two HIP events after as many untimed ones, average ms per run: path 0 = the tree on the default
// route (the switch), 1 = the tree one level per launch above the LDS stage, 2 = the whole proof as zk_gprod_prove enqueues it (no shift,
// a fixed seed; without the proof block's way to the host and its one wait).  t is left intact.
extern "C" int32_t zk_bench_gprod(zk_ctx *c, const zk_mle *t, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !t || !out_ms || reps < 1 || path < 0 || path > 2) return ZK_ERR_BAD_ARG;
    ZKCHK(gprod_table_args(c, t));
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)t->n_vars;
    const Fe sigma = fe_zero();
    if (path == kGprodPathProof) {
        const uint8_t seed[32] = {};
        DrainOnExit drain(c);
        auto once = [&]() -> int32_t {
            PoolScope ps(c);   // its blocks go back stream-ordered and come out of the pool again on the next call
            uint64_t *d_block = nullptr;
            return gprod_enqueue(c, t, sigma, seed, ps, &d_block);
        };
        ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
        drain.armed = false;   // the span has waited for ev1
        return ZK_OK;
    }
    const uint32_t fuse = path == kGprodPathDefault ? gprod_tree_fuse() : 1;
    PoolBlock heap;
    DrainOnExit drain(c);
    ZKCHK(heap.alloc(c, mle_block_bytes(n)));
    auto once = [&]() -> int32_t { return gprod_tree(c, t->d, n, false, sigma, fuse, heap.as()); };
    ZKCHK(timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms));
    drain.armed = false;
    return ZK_OK;
}
