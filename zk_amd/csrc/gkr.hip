// gkr.hip -- host side of the GKR-shaped driver (kernels: gkr_kernels.cuh); the context, table handles, prover core and verifier
// helpers it uses are declared in host_core.hpp.
//
// the reference has no gkr crate.  What it has is the building block, prove_partial / verify_partial
// (sumcheck/src/prover.rs:24-30, sumcheck/src/verifier.rs:38-41), whose doc comment names GKR as the reason the polynomial
// is NOT absorbed (evaluation_form.rs:45-48).  This driver is the layered loop a gkr crate would run on top of those calls;
// circuit format, transcript schedule and proof layout are OURS, so parity is definitional:
// tests check it against an independent big-int model (oracle/gkr_ref.py) and through the verifier below.
//
// Circuit: layers 0 (outputs) .. d-1, layer i = 2^log_out gates over the 2^log_in values of layer i+1 (layer d = inputs).
// Per layer, with E = alpha*eq(g1,.) + beta*eq(g2,.) and W = values of layer i+1 (Libra's two phases, each ONE
// prove_partial on a sum of products, D = 2):
//   claim  c = alpha*V_i(g1) + beta*V_i(g2)
//   #1 over x:  P1(x) = W(x)*H(x) + B1(x),  sum = c        -> round polys, point u, W(u), H(u), B1(u)
//   #2 over y:  P2(y) = W(y)*H2(y) + C2(y), sum = P1(u)    -> round polys, point v, W(v)
//   proof += [rp1 | rp2 | W(u) | W(v)];  transcript absorbs them, samples alpha', beta';  c' = alpha'*W(u) + beta'*W(v)
// The verifier replays the transcript, runs verify_partial twice per layer, checks
//   P2(v) == add~E(u,v)*(W(u)+W(v)) + mul~E(u,v)*W(u)*W(v)
// with the wiring predicates summed over the gate list, and finally W(u), W(v) of the input layer against the input MLE.
#include <hip/hip_runtime.h>

#include <new>
#include <utility>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "env.hpp"
#include "gkr_kernels.cuh"
#include "prover_state.hpp"


struct GkrLayer {
    uint32_t log_out, log_in;
    uint64_t n_gates, n_in;
    uint8_t *d_op;
    uint32_t *d_left, *d_right;                      // gate order
    uint32_t *d_lptr, *d_rptr;                       // CSR row pointers over the gate list by left / right input
    uint2 *d_lent, *d_rent;                          // CSR entries {z, other input | op << 31}
    uint32_t *d_lheavy, *d_rheavy;                   // rows with more than kGkrHeavyRow entries (one workgroup each)
    uint32_t n_lheavy, n_rheavy;
    // the same CSRs with the heavy rows emptied (what the entry-parallel kernels walk): aliases of the full ones when there is
    // no heavy row
    uint32_t *d_lptr_light, *d_rptr_light;
    uint2 *d_lent_light, *d_rent_light;
    uint8_t digest[112];                             // [log_out u64le | log_in u64le | tree(op) | tree(left) | tree(right)]
    // the owners of the arrays above, in upload order (gkr_upload): at most thirteen -- an alias has none, so nothing is freed twice
    RawBlock blocks[13];
    int n_blocks;
};
struct zk_circuit {
    zk_ctx *ctx;
    std::vector<GkrLayer> layers;
};

extern "C" int32_t zk_circuit_create(zk_ctx *c, zk_circuit **out) {
    if (!c || !out) return ZK_ERR_BAD_ARG;
    zk_circuit *z = new (std::nothrow) zk_circuit();
    if (!z) return ZK_ERR_ALLOC;
    z->ctx = c;
    *out = z;
    return ZK_OK;
}
extern "C" int32_t zk_circuit_free(zk_circuit *z) {
    if (!z) return ZK_OK;
    (void)use_device(z->ctx);
    delete z;   // the layers' owners free their arrays
    return ZK_OK;
}
extern "C" int32_t zk_circuit_depth(const zk_circuit *z, uint64_t *out) {
    if (!z || !out) return ZK_ERR_BAD_ARG;
    *out = z->layers.size();
    return ZK_OK;
}
extern "C" int32_t zk_circuit_layer_dims(const zk_circuit *z, uint64_t layer, uint64_t *log_out, uint64_t *log_in) {
    if (!z || layer >= z->layers.size() || !log_out || !log_in) return ZK_ERR_BAD_ARG;
    *log_out = z->layers[layer].log_out;
    *log_in = z->layers[layer].log_in;
    return ZK_OK;
}
// proof = per layer [rp #1: log_in*3 | rp #2: log_in*3 | W(u) | W(v)] elements
extern "C" int32_t zk_circuit_proof_elems(const zk_circuit *z, uint64_t *out) {
    if (!z || !out) return ZK_ERR_BAD_ARG;
    uint64_t n = 0;
    for (const auto &L : z->layers) n += 6ull * L.log_in + 2;
    *out = n;
    return ZK_OK;
}

// ---- statement digest (tree hash on the device, oracle/gkr_ref.py: tree_digest) ----------------------------------------------
// Reduce n leaf digests (device, 4 u64 each, in buf_a) to the root, ping-ponging with buf_b; the root is left at the returned
// pointer (device).  Asynchronous.
static int32_t gkr_tree_reduce(zk_ctx *c, uint64_t *buf_a, uint64_t *buf_b, uint64_t n, uint64_t **root) {
    uint64_t *cur = buf_a, *nxt = buf_b;
    while (n > 1) {
        const uint64_t n_out = (n + 3) / 4;
        if (n_out <= 4096) k_tree_level_wave<<<(uint32_t)n_out, 64, 0, c->stream>>>(cur, n, nxt);   // latency-bound levels
        else k_tree_level<<<grid_for(n_out), kBlock, 0, c->stream>>>(cur, n, n_out, nxt);
        HIPCHK(hipGetLastError());
        std::swap(cur, nxt);
        n = n_out;
    }
    *root = cur;
    return ZK_OK;
}
// digest of a table's to_bytes image -> 32 bytes at d_out (device, 4 u64).  Asynchronous; scratch comes from the pool.
static int32_t gkr_table_digest_dev(zk_ctx *c, const zk_mle *t, uint64_t *d_out) {
    const uint64_t n = 1ull << t->n_vars, n_leaves = (n + 3) / 4;
    PoolScope ps(c);
    uint64_t *a = nullptr, *b = nullptr, *root = nullptr;
    ZKCHK(ps.get((size_t)n_leaves * 32, &a));
    ZKCHK(ps.get((size_t)((n_leaves + 3) / 4) * 32, &b));
    k_tree_leaves_table<<<grid_for(n_leaves), kBlock, 0, c->stream>>>(t->d, n, n_leaves, a, c->fi->P);
    HIPCHK(hipGetLastError());
    ZKCHK(gkr_tree_reduce(c, a, b, n_leaves, &root));
    HIPCHK(hipMemcpyAsync(d_out, root, 32, hipMemcpyDeviceToDevice, c->stream));
    return ZK_OK;
}
// digest of a raw device byte array -> host (synchronises; used once per layer when the circuit is built)
static int32_t gkr_bytes_digest(zk_ctx *c, const void *d_data, uint64_t nbytes, uint8_t out[32]) {
    const uint64_t n_leaves = nbytes ? (nbytes + 127) / 128 : 1;
    PoolScope ps(c);
    uint64_t *a = nullptr, *b = nullptr, *root = nullptr;
    ZKCHK(ps.get((size_t)n_leaves * 32, &a));
    ZKCHK(ps.get((size_t)((n_leaves + 3) / 4) * 32, &b));
    k_tree_leaves_bytes<<<grid_for(n_leaves), kBlock, 0, c->stream>>>((const uint8_t *)d_data, nbytes, n_leaves, a);
    HIPCHK(hipGetLastError());
    ZKCHK(gkr_tree_reduce(c, a, b, n_leaves, &root));
    HIPCHK(hipMemcpyAsync(out, root, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
static void put_u64le(uint8_t *p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
// Keccak256 over the layers of [log_out | log_in | tree(op) | tree(left) | tree(right)]
static void gkr_circuit_digest(const zk_circuit *z, uint8_t out[32]) {
    Sponge h;
    h.init();
    for (const auto &L : z->layers) h.update(L.digest, sizeof L.digest);
    h.finalize_reset(out);
}

template <typename T>
static int32_t gkr_upload(GkrLayer &L, T **dst, const T *src, size_t count) {
    if (L.n_blocks == (int)(sizeof L.blocks / sizeof L.blocks[0])) return ZK_ERR_ALLOC;   // (cannot happen: thirteen uploads per layer)
    RawBlock b;
    HIPCHK(hipMalloc(b.put(), (count ? count : 1) * sizeof(T)));
    if (count) HIPCHK(hipMemcpy(b.get(), src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<T *>(b.get());
    L.blocks[L.n_blocks++] = std::move(b);
    return ZK_OK;
}
// CSR without its heavy rows: row pointers with those rows emptied, entries compacted
static int32_t gkr_upload_light(GkrLayer &L, const std::vector<uint32_t> &ptr, const std::vector<uint2> &ent, const std::vector<uint32_t> &heavy,
                                uint32_t *d_ptr, uint2 *d_ent, uint32_t **d_ptr_light, uint2 **d_ent_light) {
    if (heavy.empty()) {
        *d_ptr_light = d_ptr;
        *d_ent_light = d_ent;
        return ZK_OK;
    }
    const size_t rows = ptr.size() - 1;
    std::vector<uint32_t> lp(rows + 1, 0);
    std::vector<uint2> le;
    le.reserve(ent.size());
    for (size_t i = 0; i < rows; ++i) {
        if (ptr[i + 1] - ptr[i] <= kGkrHeavyRow) le.insert(le.end(), ent.begin() + ptr[i], ent.begin() + ptr[i + 1]);
        lp[i + 1] = (uint32_t)le.size();
    }
    ZKCHK(gkr_upload(L, d_ptr_light, lp.data(), lp.size()));
    return gkr_upload(L, d_ent_light, le.data(), le.size());
}
// Layers are appended from the outputs towards the inputs: layer i's log_in must equal layer i+1's log_out.
extern "C" int32_t zk_circuit_add_layer(zk_circuit *z, uint64_t log_out, uint64_t log_in, const uint8_t *op, const uint32_t *left,
                                        const uint32_t *right) {
    if (!z || !op || !left || !right) return ZK_ERR_BAD_ARG;
    if (log_in < 1 || log_in > 30 || log_out > 30) return ZK_ERR_UNSUPPORTED;   // 32-bit gate indices; >= 1 sumcheck round
    if (!z->layers.empty() && z->layers.back().log_in != log_out) return ZK_ERR_ARITY_MISMATCH;
    ZKCHK(use_device(z->ctx));
    const uint64_t n = 1ull << log_out, n_in = 1ull << log_in;
    for (uint64_t g = 0; g < n; ++g)
        if (op[g] > 1 || left[g] >= n_in || right[g] >= n_in) return ZK_ERR_BAD_ARG;
    // CSR by left and by right input (counting sort, stable in gate order)
    std::vector<uint32_t> lptr(n_in + 1, 0), rptr(n_in + 1, 0);
    std::vector<uint2> lent(n), rent(n);
    for (uint64_t g = 0; g < n; ++g) {
        ++lptr[left[g] + 1];
        ++rptr[right[g] + 1];
    }
    for (uint64_t i = 0; i < n_in; ++i) {
        lptr[i + 1] += lptr[i];
        rptr[i + 1] += rptr[i];
    }
    {
        std::vector<uint32_t> lc(lptr.begin(), lptr.end() - 1), rc(rptr.begin(), rptr.end() - 1);
        for (uint64_t g = 0; g < n; ++g) {
            const uint32_t opbit = (uint32_t)op[g] << 31;
            lent[lc[left[g]]++] = make_uint2((uint32_t)g, right[g] | opbit);
            rent[rc[right[g]]++] = make_uint2((uint32_t)g, left[g] | opbit);
        }
    }
    std::vector<uint32_t> lheavy, rheavy;
    for (uint64_t i = 0; i < n_in; ++i) {
        if (lptr[i + 1] - lptr[i] > kGkrHeavyRow) lheavy.push_back((uint32_t)i);
        if (rptr[i + 1] - rptr[i] > kGkrHeavyRow) rheavy.push_back((uint32_t)i);
    }
    GkrLayer L = {};
    L.log_out = (uint32_t)log_out;
    L.log_in = (uint32_t)log_in;
    L.n_gates = n;
    L.n_in = n_in;
    ZKCHK(gkr_upload(L, &L.d_op, op, n));
    ZKCHK(gkr_upload(L, &L.d_left, left, n));
    ZKCHK(gkr_upload(L, &L.d_right, right, n));
    ZKCHK(gkr_upload(L, &L.d_lptr, lptr.data(), lptr.size()));
    ZKCHK(gkr_upload(L, &L.d_lent, lent.data(), n));
    ZKCHK(gkr_upload(L, &L.d_rptr, rptr.data(), rptr.size()));
    ZKCHK(gkr_upload(L, &L.d_rent, rent.data(), n));
    ZKCHK(gkr_upload(L, &L.d_lheavy, lheavy.data(), lheavy.size()));
    ZKCHK(gkr_upload(L, &L.d_rheavy, rheavy.data(), rheavy.size()));
    L.n_lheavy = (uint32_t)lheavy.size();
    L.n_rheavy = (uint32_t)rheavy.size();
    ZKCHK(gkr_upload_light(L, lptr, lent, lheavy, L.d_lptr, L.d_lent, &L.d_lptr_light, &L.d_lent_light));
    ZKCHK(gkr_upload_light(L, rptr, rent, rheavy, L.d_rptr, L.d_rent, &L.d_rptr_light, &L.d_rent_light));
    // the layer's share of the statement digest (hashed from the uploaded arrays on the device)
    put_u64le(L.digest, log_out);
    put_u64le(L.digest + 8, log_in);
    ZKCHK(gkr_bytes_digest(z->ctx, L.d_op, n, L.digest + 16));
    ZKCHK(gkr_bytes_digest(z->ctx, L.d_left, n * 4, L.digest + 48));
    ZKCHK(gkr_bytes_digest(z->ctx, L.d_right, n * 4, L.digest + 80));
    z->layers.push_back(std::move(L));
    return ZK_OK;
}

// ---- eq tables -------------------------------------------------------------------------------------------------------
// out (+)= scale * eq(point, .) over m variables (variable 0 = index MSB), point in DEVICE memory: the two half tables
// (one small launch for m <= 30), then their outer product -- one multiply per element.  No host synchronisation.
static int32_t gkr_eq_table_dev(zk_ctx *c, const uint64_t *d_point, uint64_t m, const Fe &scale, bool accumulate, uint64_t *d_out,
                                const uint64_t *d_scale = nullptr /* device scalar overriding `scale` */) {
    const FieldParams &P = c->fi->P;
    const uint64_t hi_bits = m / 2, lo_bits = m - hi_bits;
    // the pool hands these blocks out again only to work enqueued later on the same stream
    PoolScope ps(c);
    uint64_t *d_hi = nullptr, *d_lo = nullptr;
    ZKCHK(ps.get((size_t)32 << hi_bits, &d_hi));
    ZKCHK(ps.get((size_t)32 << lo_bits, &d_lo));
    {
        if (m <= 30) {   // both halves in one small launch (quarter tables in LDS)
            const size_t lds = ((size_t)2 << ((lo_bits + 1) / 2)) * 32 + (size_t)2 * lo_bits * 32 + 64;
            k_eq_halves<<<2, kBlock, lds, c->stream>>>(d_point, (uint32_t)m, scale, d_hi, d_lo, P, d_scale);
        } else {
            k_eq_direct<<<grid_for(1ull << hi_bits), kBlock, 0, c->stream>>>(d_point, (uint32_t)hi_bits, scale, d_hi, P, d_scale);
            k_eq_direct<<<grid_for(1ull << lo_bits), kBlock, 0, c->stream>>>(d_point + 4 * hi_bits, (uint32_t)lo_bits, fe_one(P), d_lo, P);
        }
        if (accumulate)
            k_eq_outer<true><<<grid_for(1ull << m), kBlock, 0, c->stream>>>(d_hi, d_lo, (uint32_t)lo_bits, 1ull << m, d_out, P);
        else
            k_eq_outer<false><<<grid_for(1ull << m), kBlock, 0, c->stream>>>(d_hi, d_lo, (uint32_t)lo_bits, 1ull << m, d_out, P);
        HIPCHK(hipGetLastError());
    }
    return ZK_OK;
}
int32_t zk::eq_table_dev(zk_ctx *c, const uint64_t *d_point, uint64_t m, uint64_t *d_out) {
    return gkr_eq_table_dev(c, d_point, m, fe_one(c->fi->P), false, d_out);
}
// E = (*d_s1) * eq(p1, .) + (*d_s2) * eq(p2, .) over m <= 30 variables in one pass (points and scales in device memory)
static int32_t gkr_upload_point(zk_ctx *c, const uint64_t *point, uint64_t m, uint64_t *d_point) {
    if (m == 0) return ZK_OK;
    // the synchronise keeps the pageable source alive until the copy is done
    HIPCHK(hipMemcpyAsync(d_point, point, (size_t)m * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
// The halves of eq(p1, .) (and of eq(p2, .)) without the outer product: the GKR kernels read the table through EqFactor.
// d_s1 / d_s2: device scalars folded into the hi halves (null = 1); d_p2 == null: one point.  One launch (k_eq_split); the buffer goes back
// to the pool when its EqHalves dies or is reset(), once the kernels that read it are enqueued (stream-ordered reuse).
struct EqHalves {
    PoolBlock buf;
    EqFactor f = {};
    void reset() { buf.reset(); }
};
static int32_t gkr_eq_halves(zk_ctx *c, const uint64_t *d_p1, const uint64_t *d_s1, const uint64_t *d_p2, const uint64_t *d_s2, uint64_t m,
                             EqHalves *out) {
    const FieldParams &P = c->fi->P;
    out->reset();
    out->f = {};
    if (m > 30) return ZK_ERR_UNSUPPORTED;   // (zk_circuit_add_layer admits no such layer)
    const uint32_t lo_bits = eq_split_lo_bits(m), hi_bits = (uint32_t)m - lo_bits;
    const size_t hb = (size_t)32 << hi_bits, lb = (size_t)(kEqLoWords * 4) << lo_bits;   // lo entries are prepared multipliers
    ZKCHK(out->buf.alloc(c, (d_p2 ? 2 : 1) * (hb + lb)));
    uint64_t *hi1 = out->buf.as(), *lo1 = hi1 + hb / 8, *hi2 = d_p2 ? lo1 + lb / 8 : nullptr, *lo2 = d_p2 ? hi2 + hb / 8 : nullptr;
    const uint32_t bh = ((1u << hi_bits) + 1023) / 1024, bl = ((1u << lo_bits) + 1023) / 1024;
    const EqSplitJob j0 = {d_p1, d_s1, hi1, reinterpret_cast<uint32_t *>(lo1)}, j1 = {d_p2, d_s2, hi2, reinterpret_cast<uint32_t *>(lo2)};
    k_eq_split<<<(d_p2 ? 2 : 1) * (bh + bl), kBlock, 0, c->stream>>>(j0, j1, (uint32_t)m, lo_bits, bh, bl, P);
    HIPCHK(hipGetLastError());
    out->f = {hi1, hi2, reinterpret_cast<const uint32_t *>(lo1), reinterpret_cast<const uint32_t *>(lo2), lo_bits};
    return ZK_OK;
}
static int32_t gkr_eq_table(zk_ctx *c, const uint64_t *point, uint64_t m, const Fe *scale, bool accumulate, uint64_t *d_out) {
    PoolBlock d_point;
    ZKCHK(d_point.alloc(c, (size_t)(m ? m : 1) * 32));
    ZKCHK(gkr_upload_point(c, point, m, d_point.as()));
    return gkr_eq_table_dev(c, d_point.as(), m, scale ? *scale : fe_one(c->fi->P), accumulate, d_out);
}
// eq(point, .) as a table handle (public: the verifier of a layered protocol needs it too)
extern "C" int32_t zk_eq_table(zk_ctx *c, const uint64_t *point, uint64_t n_vars, zk_mle **out) {
    if (!c || !out || (!point && n_vars)) return ZK_ERR_BAD_ARG;
    if (n_vars > kMaxVars) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    MleHolder t;
    ZKCHK(mle_alloc(c, n_vars, t.put()));
    ZKCHK(gkr_eq_table(c, point, n_vars, nullptr, false, t->d));
    *out = t.release();
    return ZK_OK;
}

// ---- circuit evaluation ------------------------------------------------------------------------------------------------
static int32_t gkr_check_input(const zk_circuit *z, const zk_mle *input) {
    if (!z || !input) return ZK_ERR_BAD_ARG;
    if (z->layers.empty()) return ZK_ERR_BAD_ARG;
    if (input->ctx != z->ctx) return ZK_ERR_CONTEXT_MISMATCH;
    if (input->n_vars != z->layers.back().log_in) return ZK_ERR_ARITY_MISMATCH;
    return use_device(z->ctx);
}
// values of every layer: vals[d] = input (borrowed), vals[i] = own[i] for i < d
struct GkrValues {
    std::vector<MleHolder> own;
    std::vector<zk_mle *> vals;
};
static int32_t gkr_forward(const zk_circuit *z, const zk_mle *input, GkrValues &v) {
    zk_ctx *c = z->ctx;
    const size_t d = z->layers.size();
    v.own.resize(d);
    v.vals.assign(d + 1, nullptr);
    v.vals[d] = const_cast<zk_mle *>(input);
    for (size_t i = d; i-- > 0;) {
        const GkrLayer &L = z->layers[i];
        ZKCHK(mle_alloc(c, L.log_out, v.own[i].put()));
        v.vals[i] = v.own[i].get();
        k_gkr_forward<<<grid_for(L.n_gates), kBlock, 0, c->stream>>>(L.d_op, L.d_left, L.d_right, v.vals[i + 1]->d, L.n_gates, v.vals[i]->d, c->fi->P);
        HIPCHK(hipGetLastError());
    }
    return ZK_OK;
}
extern "C" int32_t zk_gkr_evaluate(const zk_circuit *z, const zk_mle *input, zk_mle **out_outputs) {
    if (!out_outputs) return ZK_ERR_BAD_ARG;
    ZKCHK(gkr_check_input(z, input));
    GkrValues v;
    ZKCHK(gkr_forward(z, input, v));
    *out_outputs = v.own[0].release();   // the inner layers go back to the pool with v
    return ZK_OK;
}

// ---- transcript helpers --------------------------------------------------------------------------------------------------
struct GkrClaim {                // alpha*V(g1) + beta*V(g2) = c;  beta == 0 on the output layer
    std::vector<uint64_t> g1, g2;
    Fe alpha, beta, c;
    bool two;
};
// The driver's transcript binds the whole statement BEFORE the output point g is drawn: the caller's seed, then the digests of
// circuit, inputs and claimed outputs (with g a function of the seed alone, outputs + delta with delta~(g) = 0 would
// have verified with the honest proof).
static int32_t gkr_start(const zk_circuit *z, const zk_mle *input, const zk_mle *outputs, Sponge &sp, const uint8_t seed[32], GkrClaim &cl) {
    zk_ctx *c = z->ctx;
    const FieldParams &P = c->fi->P;
    const uint64_t log_out0 = z->layers[0].log_out;
    uint8_t cd[32], io[64];
    gkr_circuit_digest(z, cd);
    {
        PoolBlock d_dig;
        ZKCHK(d_dig.alloc(c, 64));
        ZKCHK(gkr_table_digest_dev(c, input, d_dig.as()));
        ZKCHK(gkr_table_digest_dev(c, outputs, d_dig.as() + 4));
        HIPCHK(hipMemcpyAsync(c->h_pinned, d_dig.p, 64, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    memcpy(io, c->h_pinned, 64);
    sp.init();
    sp.update(seed, 32);
    sp.update(cd, 32);
    sp.update(io, 64);
    cl.g1.assign(4 * log_out0, 0);
    for (uint64_t i = 0; i < log_out0; ++i) fe_to_u64limbs(squeeze_field_element(sp, P), cl.g1.data() + 4 * i);
    cl.g2.clear();
    cl.alpha = fe_one(P);
    cl.beta = fe_zero();
    cl.two = false;
    return ZK_OK;
}
// E = alpha*eq(g1) + beta*eq(g2) into d_E (2^log_out elements)
// the layer's messages were absorbed as they were produced ([rp #1 | W(u)], then [rp #2 | W(v)]): draw alpha, beta
static void gkr_next_claim(Sponge &sp, const FieldParams &P, const uint64_t *layer_proof, uint64_t log_in, const uint64_t *u,
                           const uint64_t *v, GkrClaim &cl) {
    cl.alpha = squeeze_field_element(sp, P);
    cl.beta = squeeze_field_element(sp, P);
    cl.two = true;
    cl.g1.assign(u, u + 4 * log_in);
    cl.g2.assign(v, v + 4 * log_in);
    const Fe wu = fe_from_u64limbs(layer_proof + 4 * (6 * log_in)), wv = fe_from_u64limbs(layer_proof + 4 * (6 * log_in + 1));
    cl.c = fe_add(fe_mul(cl.alpha, wu, P), fe_mul(cl.beta, wv, P), P);
}

// ---- prover ----------------------------------------------------------------------------------------------------------------
// ONE transcript for the whole proof, kept on the device: after the statement (host: seed and digests -> output point g) every
// sumcheck continues the same sponge (prove_core in DeviceChain mode: the rounds only), and the scalar steps in between --
// W(u) into proof and transcript, claim of #2 = P1(u), alpha / beta, next claim -- are one-wave kernels (k_gkr_chain_*).  Points,
// claims and alpha / beta never leave the device, round polynomials are written straight into the device proof buffer: between
// the upload of g and the download of the finished proof nothing waits on the host.
extern "C" int32_t zk_gkr_prove(const zk_circuit *z, const zk_mle *input, const uint8_t seed[32], zk_mle **out_outputs,
                                uint64_t *out_proof) {
    if (!seed || !out_outputs || !out_proof) return ZK_ERR_BAD_ARG;
    ZKCHK(gkr_check_input(z, input));
    zk_ctx *c = z->ctx;
    const FieldParams &P = c->fi->P;
    const size_t d = z->layers.size();
    // declaration order is the order of the way out: the stream is waited for (drain) before the scratch (ps) and the layer
    // values (v) go back -- the download below reads d_proof, and queued kernels read all of them
    GkrValues v;
    PoolScope ps(c);
    DrainOnExit drain(c);
    ZKCHK(gkr_forward(z, input, v));
    const std::vector<zk_mle *> &vals = v.vals;
    uint64_t proof_elems = 0;
    (void)zk_circuit_proof_elems(z, &proof_elems);
    Sponge sp;
    GkrClaim cl;
    ZKCHK(gkr_start(z, input, vals[0], sp, seed, cl));
    // device state of the proof: g1, g2 of the current claim; u, v being produced; factor values of the last sumcheck; the
    // scalar block (claim, alpha, beta, claim of #2); the sponge; the proof
    constexpr size_t kPointBytes = 64 * 32;
    uint64_t *d_pt[4] = {nullptr, nullptr, nullptr, nullptr}, *d_fin = nullptr, *d_sc = nullptr, *d_proof = nullptr;
    WordSponge *d_sponge = nullptr;
    for (int i = 0; i < 4; ++i) ZKCHK(ps.get(kPointBytes, &d_pt[i]));
    ZKCHK(ps.get(kMaxFactors * 32, &d_fin));
    ZKCHK(ps.get(kGkrScalars * 32, &d_sc));
    ZKCHK(ps.get(sizeof(WordSponge), &d_sponge));
    ZKCHK(ps.get((size_t)proof_elems * 32, &d_proof));
    uint64_t *d_epart = nullptr;   // E-partial buffers + counters of the pipelined rounds, shared by all 2 * depth sumchecks
    ZKCHK(ps.get(kEpartBlockBytes, &d_epart));
    uint64_t *d_g1 = d_pt[0], *d_g2 = d_pt[1], *d_u = d_pt[2], *d_v = d_pt[3];
    ZKCHK(gkr_upload_point(c, cl.g1.data(), z->layers[0].log_out, d_g1));
    ZKCHK(sponge_to_device(c, sp, d_sponge, d_epart));
    ZKCHK(evaluate_device(c, vals[0], cl.g1.data(), d_sc + 4 * kGkrScClaim));   // claim c = V_0(g)
    k_gkr_chain_start<<<1, 64, 0, c->stream>>>(d_sponge, d_sc, P);
    HIPCHK(hipGetLastError());
    bool two = false;
    uint64_t *proof = d_proof;
    for (size_t i = 0; i < d; ++i) {
        const GkrLayer &L = z->layers[i];
        const uint64_t s = L.log_in;
        MleHolder H, B, H2, C2;   // per layer: back to the pool at the end of the iteration (the footprint at 2^24 counts on it)
        ZKCHK(mle_alloc(c, s, H.put()));
        ZKCHK(mle_alloc(c, s, B.put()));
        ZKCHK(mle_alloc(c, s, H2.put()));
        ZKCHK(mle_alloc(c, s, C2.put()));
        // E = alpha*eq(g1) + beta*eq(g2) (on the output layer just eq(g)) and, later, eq(u): as halves only (EqFactor)
        EqHalves hE, hU;
        ZKCHK(gkr_eq_halves(c, d_g1, two ? d_sc + 4 * kGkrScAlpha : nullptr, two ? d_g2 : nullptr, two ? d_sc + 4 * kGkrScBeta : nullptr, L.log_out, &hE));
        k_gkr_phase<1><<<gkr_phase_grid(L.n_in), kBlock, 0, c->stream>>>(L.d_lptr_light, L.d_lent_light, hE.f, vals[i + 1]->d, EqFactor{}, nullptr, L.n_in,
                                                                         H->d, B->d, P);
        if (L.n_lheavy) k_gkr_phase1_heavy<<<L.n_lheavy, kBlock, 0, c->stream>>>(L.d_lheavy, L.d_lptr, L.d_lent, hE.f, vals[i + 1]->d, H->d, B->d, P);
        HIPCHK(hipGetLastError());
        TermSpec ts = {2, {2, 1, 0, 0}};
        zk_mle *f1[3] = {vals[i + 1], H.get(), B.get()};
        const DeviceChain ch1 = {d_sponge, proof, d_u, d_fin, d_epart};                               // #1: over x, claim c (absorbed)
        ZKCHK(prove_core(c, f1, 3, ts, 2, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ch1));
        // W(u) -> proof, transcript; claim of #2 = P1(u) = W(u) H(u) + B1(u)
        k_gkr_chain_mid<<<1, 64, 0, c->stream>>>(d_sponge, d_fin, proof + 4 * (6 * s), d_sc, P);
        HIPCHK(hipGetLastError());
        ZKCHK(gkr_eq_halves(c, d_u, nullptr, d_u, d_fin, s, &hU));   // eq(u) twice: plain, and times W(u) = d_fin[0] (eq_u_at)
        k_gkr_phase<2><<<gkr_phase_grid(L.n_in), kBlock, 0, c->stream>>>(L.d_rptr_light, L.d_rent_light, hE.f, nullptr, hU.f, d_fin, L.n_in, H2->d, C2->d, P);
        if (L.n_rheavy) k_gkr_phase2_heavy<<<L.n_rheavy, kBlock, 0, c->stream>>>(L.d_rheavy, L.d_rptr, L.d_rent, hE.f, hU.f, d_fin, H2->d, C2->d, P);
        HIPCHK(hipGetLastError());
        hE.reset();   // stream-ordered reuse
        hU.reset();
        zk_mle *f2[3] = {vals[i + 1], H2.get(), C2.get()};
        const DeviceChain ch2 = {d_sponge, proof + 4 * (3 * s), d_v, d_fin, d_epart};                 // #2: over y, claim P1(u) (absorbed)
        ZKCHK(prove_core(c, f2, 3, ts, 2, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ch2));
        // W(v) -> proof, transcript; alpha, beta; next claim (absorbed as the next sumcheck's first message)
        k_gkr_chain_end<<<1, 64, 0, c->stream>>>(d_sponge, d_fin, proof + 4 * (6 * s), proof + 4 * (6 * s + 1), d_sc, P);
        HIPCHK(hipGetLastError());
        proof += 4 * (6 * s + 2);
        std::swap(d_g1, d_u);   // the next layer's claim sits at (u, v)
        std::swap(d_g2, d_v);
        two = true;
    }
    // the one download of the proof (pageable destination: the copy is synchronous with respect to the host)
    HIPCHK(hipMemcpyAsync(out_proof, d_proof, (size_t)proof_elems * 32, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    *out_outputs = v.own[0].release();
    return ZK_OK;
}

// ---- verifier ------------------------------------------------------------------------------------------------------------
// ZK_OK = accept.  ZK_ERR_VERIFY_SUM = a sumcheck round check failed (verifier.rs:64 text); ZK_ERR_GKR_REJECT = a layer's
// wiring check or the final input check failed.
// The transcript replay (host: the round checks of both sumchecks of a layer, W(u), W(v), alpha, beta) needs nothing from the
// device -- the wiring predicates are not transcript input -- so the device never makes the host wait inside the layer loop:
// as soon as a layer's points exist they go up (one async copy out of pinned memory) and its E / eq_u / eq_v tables and wiring
// sums are enqueued, while the host replays the next layer.  The 2 * depth predicate values come back in one copy at the end:
// ONE host wait for the whole circuit instead of five per layer.  A failed round check rejects at once; the wiring checks are
// compared afterwards, so a proof with several defects is rejected by the first check in THAT order.
struct GkrLayerCheck {
    Fe sub2, wu, wv;
};
extern "C" int32_t zk_gkr_verify(const zk_circuit *z, const zk_mle *input, const zk_mle *outputs, const uint8_t seed[32],
                                 const uint64_t *proof_in) {
    if (!seed || !outputs || !proof_in) return ZK_ERR_BAD_ARG;
    ZKCHK(gkr_check_input(z, input));
    zk_ctx *c = z->ctx;
    if (outputs->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (outputs->n_vars != z->layers[0].log_out) return ZK_ERR_ARITY_MISMATCH;
    const FieldParams &P = c->fi->P;
    const size_t d = z->layers.size();
    Sponge sp;
    GkrClaim cl;
    ZKCHK(gkr_start(z, input, outputs, sp, seed, cl));
    uint64_t ev[4];
    ZKCHK(zk_mle_evaluate(c, outputs, cl.g1.data(), z->layers[0].log_out, ev));
    cl.c = fe_from_u64limbs(ev);
    const uint64_t *proof = proof_in;
    std::vector<GkrLayerCheck> chk(d);
    size_t words = 0;   // uint64 words of the point block: per layer [g1 | g2 | u | v | alpha | beta]
    for (size_t i = 0; i < d; ++i) words += 4 * (2 * (size_t)z->layers[i].log_out + 2 * (size_t)z->layers[i].log_in + 2);
    uint8_t *stage = nullptr;
    ZKCHK(results_staging(c, words * 8 + d * 64, &stage));
    uint64_t *h_blk = reinterpret_cast<uint64_t *>(stage), *h_pred = h_blk + words;
    std::vector<uint64_t> u, v;
    {
        // the way out of this block, early or not, waits for the stream (drain) before d_blk / d_pred go back (ps): the copies out
        // of the pinned block and the kernels reading d_blk must be done before either is reused
        PoolScope ps(c);
        DrainOnExit drain(c);
        uint64_t *d_blk = nullptr, *d_pred = nullptr;
        ZKCHK(ps.get(words * 8, &d_blk));
        ZKCHK(ps.get(d * 64, &d_pred));
        size_t at = 0;
        for (size_t i = 0; i < d; ++i) {
            const GkrLayer &L = z->layers[i];
            const uint64_t s = L.log_in;
            const size_t lo4 = 4 * (size_t)L.log_out;
            GkrLayerCheck &k = chk[i];
            // this layer's slice of the point block; the claim it starts from first (the replay below replaces cl)
            uint64_t *w = h_blk + at;
            const bool two = cl.two;
            memcpy(w, cl.g1.data(), lo4 * 8);
            if (two) memcpy(w + lo4, cl.g2.data(), lo4 * 8);
            else memset(w + lo4, 0, lo4 * 8);
            fe_to_u64limbs(cl.alpha, w + 2 * lo4 + 8 * s);
            fe_to_u64limbs(cl.beta, w + 2 * lo4 + 8 * s + 4);
            u.assign(4 * s, 0);
            v.assign(4 * s, 0);
            uint64_t sum[4];
            Fe sub1;
            fe_to_u64limbs(cl.c, sum);
            ZKCHK(verify_internal(P, sp, s, 2, sum, proof, sub1, u.data()));   // the sumcheck continues the ONE driver transcript
            absorb_elements(sp, proof + 4 * (6 * s), 1, P);                    // W(u)
            fe_to_u64limbs(sub1, sum);
            ZKCHK(verify_internal(P, sp, s, 2, sum, proof + 4 * (3 * s), k.sub2, v.data()));
            absorb_elements(sp, proof + 4 * (6 * s + 1), 1, P);                // W(v)
            k.wu = fe_from_u64limbs(proof + 4 * (6 * s));
            k.wv = fe_from_u64limbs(proof + 4 * (6 * s + 1));
            memcpy(w + 2 * lo4, u.data(), 4 * s * 8);
            memcpy(w + 2 * lo4 + 4 * s, v.data(), 4 * s * 8);
            const size_t layer_words = 2 * lo4 + 8 * s + 8;
            // wiring predicates at (u, v) over the gate list: enqueued, not waited for
            uint64_t *dw = d_blk + at;
            at += layer_words;
            HIPCHK(hipMemcpyAsync(dw, w, layer_words * 8, hipMemcpyHostToDevice, c->stream));
            const uint64_t *d_g1 = dw, *d_g2 = dw + lo4, *d_u = dw + 2 * lo4, *d_v = d_u + 4 * s, *d_alpha = d_v + 4 * s, *d_beta = d_alpha + 4;
            EqHalves hE, hUV;   // E = alpha*eq(g1) + beta*eq(g2) as the prover builds it; eq(u) and eq(v) in one launch; stream-ordered reuse
            ZKCHK(gkr_eq_halves(c, d_g1, d_alpha, two ? d_g2 : nullptr, two ? d_beta : nullptr, L.log_out, &hE));
            ZKCHK(gkr_eq_halves(c, d_u, nullptr, d_v, nullptr, s, &hUV));
            const EqFactor fu = {hUV.f.hi, nullptr, hUV.f.lo, nullptr, hUV.f.lo_bits}, fv = {hUV.f.hi2, nullptr, hUV.f.lo2, nullptr, hUV.f.lo_bits};
            const uint32_t g = grid_for(L.n_gates);
            k_gkr_wiring_eval<<<g, kBlock, 0, c->stream>>>(L.d_op, L.d_left, L.d_right, hE.f, fu, fv, L.n_gates, c->d_partials, P);
            ZKCHK(launch_reduce_tail(c, g, 2, d_pred + 8 * i));
            gkr_next_claim(sp, P, proof, s, u.data(), v.data(), cl);
            proof += 4 * (6 * s + 2);
        }
        HIPCHK(hipMemcpyAsync(h_pred, d_pred, d * 64, hipMemcpyDeviceToHost, c->stream));
        ZKCHK(drain.wait());
    }
    for (size_t i = 0; i < d; ++i) {
        const GkrLayerCheck &k = chk[i];
        const Fe add_e = fe_from_u64limbs(h_pred + 8 * i), mul_e = fe_from_u64limbs(h_pred + 8 * i + 4);
        const Fe want = fe_add(fe_mul(add_e, fe_add(k.wu, k.wv, P), P), fe_mul(mul_e, fe_mul(k.wu, k.wv, P), P), P);
        if (!fe_eq(want, k.sub2)) return ZK_ERR_GKR_REJECT;
    }
    // input layer: W(u), W(v) are evaluations of the input MLE
    const uint64_t s = z->layers.back().log_in;
    const uint64_t *last = proof - 4 * (6 * s + 2);
    uint64_t eu[4], evv[4];
    ZKCHK(zk_mle_evaluate(c, input, u.data(), s, eu));
    ZKCHK(zk_mle_evaluate(c, input, v.data(), s, evv));
    if (!fe_eq(fe_from_u64limbs(eu), fe_from_u64limbs(last + 4 * (6 * s))) ||
        !fe_eq(fe_from_u64limbs(evv), fe_from_u64limbs(last + 4 * (6 * s + 1))))
        return ZK_ERR_GKR_REJECT;
    return ZK_OK;
}

// ---- pieces of the multi-GPU four-step NTT (zk_amd/distributed.py: ShardedNtt) ----------------------------------------------
// t[j] *= scale * base^j
extern "C" int32_t zk_mle_mul_powers(zk_ctx *c, zk_mle *t, const uint64_t base[4], const uint64_t scale[4]) {
    if (!c || !t || !base || !scale) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    const FieldParams &P = c->fi->P;
    const uint64_t n = 1ull << t->n_vars;
    uint32_t g = grid_for((n + 15) / 16);   // >= 16 elements per thread amortise the exponentiation
    const uint64_t stride = (uint64_t)g * kBlock;
    const Fe b = fe_from_u64limbs(base);
    k_mul_powers<<<g, kBlock, 0, c->stream>>>(t->d, n, b, fe_from_u64limbs(scale), fe_pow_u64(b, stride, P), P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// in, out: tables of log_w + log_l variables read as W rows of L = 2^log_l elements; out[k][j] = sum_r w^(r*k) in[r][j] with
// w = get_root_of_unity(W) (fft/src/lib.rs:6), or its inverse (no 1/W scaling) when inverse != 0.
extern "C" int32_t zk_dft_across(zk_ctx *c, const zk_mle *in, zk_mle *out, uint64_t log_w, int32_t inverse) {
    if (!c || !in || !out) return ZK_ERR_BAD_ARG;
    if (in->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (in->n_vars != out->n_vars || in->d == out->d || log_w > in->n_vars || log_w > 10) return ZK_ERR_BAD_ARG;
    Fe w;
    if (!field_root_of_unity(*c->fi, (uint32_t)log_w, w)) return ZK_ERR_FFT_NO_ROOT;
    ZKCHK(use_device(c));
    const FieldParams &P = c->fi->P;
    if (inverse) w = fe_inverse(w, P);
    const uint32_t W = 1u << log_w;
    const uint64_t L = 1ull << (in->n_vars - log_w);
    std::vector<uint64_t> pw(4 * (size_t)W);
    Fe cur = fe_one(P);
    for (uint32_t e = 0; e < W; ++e) {
        fe_to_u64limbs(cur, pw.data() + 4 * e);
        cur = fe_mul(cur, w, P);
    }
    PoolBlock d_pw;   // stream-ordered reuse when the call returns
    ZKCHK(d_pw.alloc(c, (size_t)W * 32));
    HIPCHK(hipMemcpyAsync(d_pw.p, pw.data(), (size_t)W * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    k_dft_across<<<grid_for(L), kBlock, 0, c->stream>>>(in->d, out->d, W, L, d_pw.as(), P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
