// host_core.hpp -- what the host units of libzk_amd.so share (capi.hip, sumcheck.hip, ntt.hip, gkr.hip, cmle.hip, inv.hip, merkle.hip, fri.hip, pcs.hip, mlpcs.hip, mlbatch.hip, gprod.hip, fsum.hip, comm.hip): the objects
// behind the C handles, the status macros, the owners of device blocks, the per-call helpers (inline) and the declarations of the few
// functions that cross units (namespace zk: none of them joins the C ABI).  No kernel is defined here or in anything this includes.
// timing.hpp, on top of this header, holds the last kind of owner: the events and timed spans of the zk_bench_* measurement hooks.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_field.hpp"
#include "keccak.hpp"
#include "launch.hpp"
#include "ntt_plan.hpp"

using namespace zk;   // (an internal header: only the library's own host units include it)

// ------------------------------------------------------------------------------------------------------------
// objects
// ------------------------------------------------------------------------------------------------------------
struct zk_ctx {
    int field;
    int device;
    const FieldInfo *fi;
    hipStream_t own_stream;
    hipStream_t stream;
    uint64_t *d_partials;   // per-block partial sums of a round: kMaxGrid * kMaxSums elements
    uint64_t *d_sums;       // final round sums (kMaxSums elements) + lanes area
    uint64_t *h_pinned;     // pinned staging: kMaxSums*8 u64
    uint32_t *h_flag;       // completion word in pinned memory: the last kernel of a call stores flag_seq there (host_flag_wait)
    uint32_t flag_seq;
    uint8_t *h_results;     // pinned staging for proofs (grown on demand)
    std::map<uint32_t, uint64_t *> lagrange_w;   // interp_weights(D) in device memory, cached (a field inversion per node)
    size_t h_results_bytes;
    hipEvent_t ev0, ev1;
    std::map<std::pair<uint32_t, int>, uint64_t *> twiddles;   // (log_n, inverse) -> omega^i table, i < n/2 (n < 2^8 path)
    std::map<std::pair<uint32_t, int>, NttPlan> ntt_plans;     // (log_n, inverse) -> pass plan + two-level twiddle tables
    std::map<size_t, std::vector<void *>> pool;                // freed device blocks by exact size (stream-ordered reuse)
    size_t pool_bytes, pool_checked;
    Fe inv2;                // 1/2 (pipelined rounds interpolate on the nodes 0, 1, -1, inf)
    PipeConsts pipe_consts; // its prepared multiplier + the constant 2^266 mod p (pipe_kernels.cuh pipe_eval_canon)
    uint64_t *d_dbg;        // ZK_PIPE_DEBUG: phase timestamps of the pipelined launches (64 launches x 32 slots + finisher)
    uint32_t dbg_launch;
    uint8_t *h_absorb[2];   // pinned staging of absorb_tables (prove / verify), kept across calls
    size_t h_absorb_bytes;
    hipEvent_t ev_absorb[2];
};
struct zk_mle {
    zk_ctx *ctx;
    uint64_t n_vars;
    uint64_t *d;
};
struct zk_upoly {   // UnivariatePolynomial (univariate_poly.rs:7-12): len coefficients, lowest degree first
    zk_ctx *ctx;
    uint64_t len;
    uint64_t *d;    // a pool block of the next power of two >= len elements (shared size classes with the tables)
};

constexpr uint32_t kMaxGrid = 2048;    // round kernels: 8 workgroups per CU on 256 CUs (partials are sized for it)
constexpr uint32_t kMaxGridStream = 16384;   // pure streaming kernels (fold): measured +10% over 2048 at 2^24
constexpr uint32_t kMaxSums = 256;     // max_var_degree is a u8 in the reference (prover.rs:9)
constexpr uint64_t kMaxVars = 40;

namespace zk {
extern thread_local std::string g_hip_err;   // ONE per thread for the whole library (defined in capi.hip): zk_last_hip_error reads it
}  // namespace zk

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess) {                                                          \
            g_hip_err = std::string(#expr) + ": " + hipGetErrorString(e__);               \
            return ZK_ERR_HIP;                                                            \
        }                                                                                 \
    } while (0)
#define ZKCHK(expr)                        \
    do {                                   \
        int32_t rc__ = (expr);             \
        if (rc__ != ZK_OK) return rc__;    \
    } while (0)

inline uint32_t grid_for(uint64_t items) {
    uint64_t b = (items + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    if (b > kMaxGrid) b = kMaxGrid;
    return (uint32_t)b;
}
// Wait for the stream.  (Until round 3 this spun on hipStreamQuery first; tools/mb/mb_flag.hip: that costs 2-4 us MORE than
// hipStreamSynchronize for kernels of 1 us .. 1.2 ms, and a completion word in pinned memory -- host_flag_wait below -- 5 us less.)
inline hipError_t stream_wait(hipStream_t s) { return hipStreamSynchronize(s); }
// ---- completion word in pinned host memory -----------------------------------------------------------------------------------
// The last kernel of a call copies the results into pinned host memory itself and then stores a sequence number next to them
// (system-scope fence in between); the host spins on that word instead of waiting for the stream's completion signal, which
// arrives ~5 us later (tools/mb/mb_flag.hip: launch + wait of a 1-us kernel 11.7 us with hipStreamSynchronize, 6.9 us with the
// word).  The stream itself is checked every few thousand spins so that a failed launch ends the wait with its error.
constexpr unsigned kPolledHostFlags = hipHostMallocCoherent | hipHostMallocMapped;
// next completion sequence number; 0 is reserved ("this launch writes no word"), so it is skipped when the counter wraps
inline uint32_t next_flag_seq(zk_ctx *c) {
    if (++c->flag_seq == 0) ++c->flag_seq;
    return c->flag_seq;
}
inline int32_t host_flag_wait(zk_ctx *c, uint32_t seq, uint32_t slot = 0) {
    volatile uint32_t *flag = c->h_flag + 16 * slot;
    for (uint32_t spins = 1;; ++spins) {
        if (*flag == seq) break;
        if ((spins & 0x3FFF) == 0) {
            const hipError_t e = hipStreamQuery(c->stream);
            if (e == hipSuccess) break;                  // the stream has drained: the kernel's stores are visible
            if (e != hipErrorNotReady) {
                g_hip_err = std::string("stream failed while waiting for the completion word: ") + hipGetErrorString(e);
                return ZK_ERR_HIP;
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return ZK_OK;
}
inline int32_t use_device(const zk_ctx *ctx) {
    HIPCHK(hipSetDevice(ctx->device));
    return ZK_OK;
}
namespace zk {
// the per-context pool of device blocks (capi.hip)
int32_t raw_alloc(zk_ctx *c, size_t bytes, void **out);
int32_t pool_alloc(zk_ctx *c, size_t bytes, void **out);
void pool_free(zk_ctx *c, void *ptr, size_t bytes);
}  // namespace zk
// ---- who owns a device block ----------------------------------------------------------------------------------------------------
// Move-only owner of ONE pool block.  It records the context and the byte count of the allocation, so the block goes back under
// exactly that size when the owner dies (stream-ordered, like every pool_free).  release() hands the block on to a longer-lived
// object (a table / polynomial handle, zk_ctx_device_alloc's caller).
struct PoolBlock {
    zk_ctx *c = nullptr;
    void *p = nullptr;
    size_t bytes = 0;
    PoolBlock() = default;
    PoolBlock(PoolBlock &&o) noexcept : c(o.c), p(o.p), bytes(o.bytes) { o.p = nullptr; }
    PoolBlock &operator=(PoolBlock &&o) noexcept {
        if (this != &o) {
            reset();
            c = o.c, p = o.p, bytes = o.bytes;
            o.p = nullptr;
        }
        return *this;
    }
    PoolBlock(const PoolBlock &) = delete;
    PoolBlock &operator=(const PoolBlock &) = delete;
    ~PoolBlock() { reset(); }
    int32_t alloc(zk_ctx *cc, size_t n) {
        reset();
        void *q = nullptr;
        ZKCHK(pool_alloc(cc, n, &q));
        c = cc, p = q, bytes = n;
        return ZK_OK;
    }
    void reset() {
        if (p) pool_free(c, p, bytes);
        p = nullptr;
    }
    void *release() {
        void *q = p;
        p = nullptr;
        return q;
    }
    template <class T = uint64_t>
    T *as() const { return static_cast<T *>(p); }
    explicit operator bool() const { return p != nullptr; }
};
// The pool blocks of one call, all handed back (stream-ordered, in allocation order) when it returns.  Inline and fixed: no heap
// allocation and no lookup per block; the capacity covers the largest user (interpolate_xy: weights, tree levels and block merges).
struct PoolScope {
    static constexpr int kCapacity = 24;
    zk_ctx *c;
    int n = 0;
    void *ptr[kCapacity];
    size_t bytes[kCapacity];
    explicit PoolScope(zk_ctx *cc) : c(cc) {}
    PoolScope(const PoolScope &) = delete;
    PoolScope &operator=(const PoolScope &) = delete;
    ~PoolScope() {
        for (int i = 0; i < n; ++i) pool_free(c, ptr[i], bytes[i]);
    }
    template <class T>
    int32_t get(size_t nbytes, T **out) {
        if (n == kCapacity) return ZK_ERR_ALLOC;   // (a new user with more blocks than the largest one: raise kCapacity)
        void *q = nullptr;
        ZKCHK(pool_alloc(c, nbytes, &q));
        ptr[n] = q, bytes[n] = nbytes;
        ++n;
        *out = static_cast<T *>(q);
        return ZK_OK;
    }
};
// Scoped holder of a temporary that one function releases: table / polynomial handles (MleHolder below, ntt.hip's UpolyHolder) and the few
// blocks that bypass the pool (RawBlock: hipFree).  put() is the out-parameter of the call that creates it.
template <class T, void (*Del)(T *)>
struct Scoped {
    T *h = nullptr;
    Scoped() = default;
    explicit Scoped(T *t) : h(t) {}
    Scoped(Scoped &&o) noexcept : h(o.release()) {}
    Scoped &operator=(Scoped &&o) noexcept {
        if (this != &o) {
            reset();
            h = o.release();
        }
        return *this;
    }
    Scoped(const Scoped &) = delete;
    Scoped &operator=(const Scoped &) = delete;
    ~Scoped() { reset(); }
    void reset() {
        if (h) Del(h);
        h = nullptr;
    }
    T *release() {
        T *t = h;
        h = nullptr;
        return t;
    }
    T **put() {
        reset();
        return &h;
    }
    T *get() const { return h; }
    T *operator->() const { return h; }
};
inline void raw_release(void *p) { (void)hipFree(p); }
using RawBlock = Scoped<void, raw_release>;
// Waits for the stream when a call leaves early, BEFORE the owners declared above it give their blocks back: for calls whose
// pinned staging or device blocks are read by work that may still be queued.  The success path waits through wait() and sees
// the status.
struct DrainOnExit {
    zk_ctx *c;
    bool armed = true;
    explicit DrainOnExit(zk_ctx *cc) : c(cc) {}
    DrainOnExit(const DrainOnExit &) = delete;
    DrainOnExit &operator=(const DrainOnExit &) = delete;
    ~DrainOnExit() {
        if (armed) (void)hipStreamSynchronize(c->stream);
    }
    int32_t wait() {
        armed = false;
        HIPCHK(hipStreamSynchronize(c->stream));
        return ZK_OK;
    }
};

// ---- the functions that cross units (every other function of a unit is static) ---------------------------------------------------
inline size_t mle_block_bytes(uint64_t n_vars) { return (size_t)32 << n_vars; }
struct DeviceChain;   // prover_state.hpp
namespace zk {
// capi.hip
int32_t mle_alloc(zk_ctx *c, uint64_t n_vars, zk_mle **out);
void mle_release(zk_mle *t);
int32_t evaluate_device(zk_ctx *c, const zk_mle *t, const uint64_t *point, uint64_t *d_out_elem, uint32_t flag_seq = 0);
int32_t host_staging(zk_ctx *c, size_t cb);
int32_t results_staging(zk_ctx *c, size_t bytes, uint8_t **out);
// consume(host_ptr, bytes): once per 16-MiB chunk of to_bytes() of the k tables, in order, on the calling thread
int32_t stream_table_bytes(zk_ctx *c, const zk_mle *const *f, uint64_t k, const std::function<void(const uint8_t *, size_t)> &consume);
uint32_t log2_world(uint32_t world);
int32_t shard_interleave(zk_ctx *c, const std::vector<uint64_t *> &ptrs, uint64_t *major, uint32_t world, uint64_t m, zk_mle **out);
// ProductPoly::new's checks (product_poly.rs:14-32) on k handles of context c, then use_device(c)
int32_t product_args(zk_ctx *c, const zk_mle *const *f, uint64_t k);
void absorb_elements(Sponge &sp, const uint64_t *elems, uint64_t n, const FieldParams &P);
Fe squeeze_field_element(Sponge &sp, const FieldParams &P);
// sumcheck.hip
int32_t sponge_to_device(zk_ctx *c, const Sponge &host, WordSponge *d_sponge, uint64_t *d_epart);
int32_t prove_core(zk_ctx *c, zk_mle *const *f, uint64_t k, const TermSpec &ts, uint32_t D, const uint64_t sum[4], int32_t absorb_table,
                   int32_t consume, uint64_t *out_rp, uint64_t *out_ch, uint64_t *out_final, uint64_t *d_keep_ch = nullptr,
                   uint64_t *d_keep_final = nullptr, const Sponge *init = nullptr, const DeviceChain *chain = nullptr);
int32_t verify_internal(const FieldParams &P, Sponge &sp, uint64_t n_rounds, const uint32_t *lens, uint32_t uniform_len, const uint64_t sum[4],
                        const uint64_t *rps, Fe &claimed, uint64_t *out_ch);
int32_t verify_internal(const FieldParams &P, Sponge &sp, uint64_t n_rounds, uint32_t D, const uint64_t sum[4], const uint64_t *rps, Fe &claimed,
                        uint64_t *out_ch);
// the second stage of a round on its own (k_round_tail without a transcript step): the nblocks x ns block partials in the context's
// buffer -> ns sums at out_rp
int32_t launch_reduce_tail(zk_ctx *c, uint32_t nblocks, uint32_t ns, uint64_t *out_rp);
// ntt.hip: a vector handle of `len` elements on a pool block of the next power of two (inv.hip makes its results with it)
int32_t upoly_alloc(zk_ctx *c, uint64_t len, zk_upoly **out);
void upoly_release(zk_upoly *p);
// merkle.hip: every level of the tree over 2^n rows of k columns given as raw device pointers into `tree`, a block of 64 << n bytes (fri.hip
// commits to a layer's 2^a column views with it)
int32_t merkle_build_raw(zk_ctx *c, const uint64_t *const *cols, uint32_t k, uint32_t n, uint64_t *tree);
// fri.hip, for pcs.hip: an element as it crosses the ABI that is fully reduced; a 32-byte big-endian canonical integer -> Montgomery
// (false: not below p); the coset LDE of p into a table of log_n variables; the prover from a given layer 0 with one more committed
// table (FRI's row layout: 2^log_m0 rows of `width` columns at stride 2^log_m0) opened at the same query indices; the verifier, which
// hands the query indices back
bool fri_elem(const uint64_t l[4], const FieldParams &P, Fe *out);
bool fri_from_be32(const uint8_t *b, const FieldParams &P, Fe *out);
int32_t fri_lde_into(zk_ctx *c, const zk_upoly *p, uint32_t log_n, const uint64_t shift[4], zk_mle *out);
struct FriTraceOpen {
    const uint64_t *table, *tree;
    uint32_t width;
    std::vector<uint64_t> staged;   // out: Q rows of `width` elements (Montgomery), then Q paths of log_m0 digests
};
int32_t fri_prove_layer0(zk_ctx *c, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final, uint32_t n_queries,
                         const Fe &shift, const uint8_t seed[32], const zk_mle *layer0, uint8_t *out_proof, uint64_t *out_idx, FriTraceOpen *trace);
int32_t fri_verify_core(int32_t field, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final, uint32_t n_queries,
                        const uint64_t shift[4], const uint8_t seed[32], const uint8_t *proof, uint64_t proof_len, int32_t *out_ok,
                        uint64_t *out_idx);
// fri.hip, for mlpcs.hip, whose opening runs the prover's rounds itself (a sumcheck launch joins every round's download): the power
// table of a domain; the fold by 2 of layer `round` (2^n points, n = log_domain - round) at beta; k_fri_gather's launch; a query index;
// the verifier's fold of one row
struct FriFoldPlan;
int32_t fri_fold_plan(zk_ctx *c, uint32_t log_domain, FriFoldPlan **out);
void fri_fold_plan_release(FriFoldPlan *pl);
int32_t fri_fold2(zk_ctx *c, const FriFoldPlan *pl, const uint64_t *in, uint32_t n, uint32_t round, const Fe &s_inv, const Fe &beta, uint64_t *out);
int32_t fri_gather(zk_ctx *c, const uint64_t *layer, const uint64_t *tree, uint32_t log_m, uint32_t width, const uint64_t *d_idx, uint32_t n_queries,
                   uint64_t *rows, uint64_t *paths);
// (for mlbatch.hip, whose first fold is a kernel of its own: the plan's power table, lo of 2^lo_bits and hi of 2^hi_bits entries)
void fri_fold_plan_table(const FriFoldPlan *pl, const uint64_t **lo, const uint64_t **hi, uint32_t *lo_bits, uint32_t *hi_bits);
uint64_t fri_query_index(Sponge &sp, uint32_t log_m0);
Fe fri_fold_row(Fe *v, uint32_t a, Fe x_inv, Fe beta, const Fe &half, const FieldInfo &fi);
// cmle.hip: zk_cmle_interpolate's transform of a table of n_vars >= 1 variables into a block of the caller's (2^n_vars coefficients)
int32_t cmle_interpolate_into(zk_ctx *c, const zk_mle *values, uint64_t *d_coeffs);
// sumcheck.hip: zk_round_sums without its download: the D + 1 sums are left at *d_out (the context's, valid until its next round)
int32_t round_sums_enqueue(zk_ctx *c, const zk_mle *const *f, uint64_t k, uint32_t D, const uint64_t **d_out);
// for gprod.hip and fsum.hip, whose proofs chain one sumcheck per layer on a device-resident transcript: gkr.hip's eq(point, .) over m variables from a
// point in DEVICE memory into d_out (the kernels behind zk_eq_table; no host wait); sumcheck.hip's k_publish_host launch (n_u64 words of a
// device block to pinned host memory, then the completion word `seq`: host_flag_wait)
int32_t eq_table_dev(zk_ctx *c, const uint64_t *d_point, uint64_t m, uint64_t *d_out);
int32_t publish_host(zk_ctx *c, const uint64_t *d_src, uint64_t *h_dst, uint32_t n_u64, uint32_t seq);
// gprod.hip, for perm.hip, whose fingerprint kernel writes level n itself and starts the tree: the switch ZK_GPROD_TREE_FUSE; heap <- the
// tree over src + sigma (2^n elements), `fuse` levels per launch above the LDS stage; a proof's scratch; the layers of a proof over a
// queued tree (the block [2 n^2 proof elements | P | r_n | c_n - sigma] is left at s.block).  All asynchronous
struct GprodScratch {
    uint64_t *heap = nullptr, *d_pt[2] = {nullptr, nullptr}, *d_fin = nullptr, *d_claim = nullptr, *d_epart = nullptr, *block = nullptr;
    WordSponge *d_sponge = nullptr;
};
uint32_t gprod_tree_fuse();
uint32_t gprod_lds_vars();   // kPtreeLdsVars: a level of at most 2^this elements goes to the one-workgroup stage
int32_t gprod_tree(zk_ctx *c, const uint64_t *src, uint32_t n, bool shift, const Fe &sigma, uint32_t fuse, uint64_t *heap);
int32_t gprod_scratch(PoolScope &ps, uint32_t n, GprodScratch *s);
int32_t gprod_layers(zk_ctx *c, uint32_t n, const uint64_t *top, const GprodScratch &s, const Fe &sigma, const uint8_t seed[32]);
}  // namespace zk
using MleHolder = Scoped<zk_mle, mle_release>;
using UpolyHolder = Scoped<zk_upoly, upoly_release>;
