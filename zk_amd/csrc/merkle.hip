// merkle.hip -- host side of the binary Keccak-256 Merkle commitments over tables (kernels in merkle_kernels.cuh; no reference item,
// definition: tests/merkle_ref.py).  The handle owns ONE pool block with every level; scratch (the column
// pointer table, the staging of an opening) comes from the context's pool and goes back stream-ordered.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "merkle_kernels.cuh"

struct zk_merkle {
    zk_ctx *ctx;
    uint32_t n_vars, n_columns;
    PoolBlock tree;   // level 0, level 1, ..., the root: 2^(n+1) - 1 digests (merkle_level_offset)
};
static void merkle_release(zk_merkle *m) { delete m; }   // the block goes back to the pool with its owner
using MerkleHolder = Scoped<zk_merkle, merkle_release>;

// ZK_MERKLE_FUSE_LEVELS: 0 = one launch per level, s = fused stages over tiles of 2^s digests.  The default is what
// profiles/merkle.log shows faster at both 2^20 and 2^24 rows.
constexpr uint32_t kMerkleFuseChosen = 10;    // the tile of the fused path when nothing else is asked for
constexpr uint32_t kMerkleFuseDefault = 0;
static uint32_t merkle_fuse_levels() {
    static const uint32_t s = (uint32_t)env_u64("ZK_MERKLE_FUSE_LEVELS", kMerkleFuseDefault, 0, kMerkleMaxTileLog);
    return s;
}
enum { kMerklePathDefault = 0, kMerklePathFused = 1, kMerklePathLevels = 2 };
// the upper levels of the level-by-level path with at most this many nodes take one wave per node (gkr.hip's statement digest made the
// same choice for the same permutation)
constexpr uint64_t kMerkleWaveMax = 4096;
constexpr uint32_t kMerkleMaxGrid = 65536;

// the block is sized as 2^(n+1) digests, one more than the tree has: the pool hands blocks out by exact size, and this is the size
// class of a table of n + 1 variables
static size_t merkle_block_bytes(uint32_t n) { return (size_t)64 << n; }
static size_t scratch_bytes(size_t bytes) {
    size_t b = 32;
    while (b < bytes) b <<= 1;
    return b;
}

// NULLs and k == 0 -> BAD_ARG; another context's handle -> CONTEXT_MISMATCH; differing n_vars -> ARITY_MISMATCH; k > 1024 -> UNSUPPORTED
static int32_t check_columns(const zk_ctx *c, const zk_mle *const *columns, uint32_t k) {
    if (!c || !columns || k == 0) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (!columns[j]) return ZK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < k; ++j)
        if (columns[j]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    for (uint32_t j = 1; j < k; ++j)
        if (columns[j]->n_vars != columns[0]->n_vars) return ZK_ERR_ARITY_MISMATCH;
    if (k > kMerkleMaxColumns) return ZK_ERR_UNSUPPORTED;
    return ZK_OK;
}
// the device array of the k column pointers, filled by launches that carry them in their arguments (no host copy to wait for)
static int32_t put_column_ptrs(zk_ctx *c, PoolScope &ps, const zk_mle *const *columns, uint32_t k, const uint64_t *const **out) {
    const uint64_t **table = nullptr;
    ZKCHK(ps.get(scratch_bytes((size_t)k * sizeof(uint64_t *)), &table));
    for (uint32_t base = 0; base < k; base += kMerklePtrBatch) {
        MerklePtrs b = {};
        const uint32_t count = k - base < kMerklePtrBatch ? k - base : kMerklePtrBatch;
        for (uint32_t j = 0; j < count; ++j) b.p[j] = columns[base + j]->d;
        k_merkle_put_ptrs<<<1, 64, 0, c->stream>>>(table, base, count, b);
    }
    HIPCHK(hipGetLastError());
    *out = table;
    return ZK_OK;
}
// every level of the tree over 2^n rows of k columns into `tree`.  Enqueues only.
static int32_t merkle_build(zk_ctx *c, const uint64_t *const *cols, uint32_t k, uint32_t n, uint64_t *tree, int path) {
    const FieldParams &P = c->fi->P;
    uint32_t fuse = path == kMerklePathLevels ? 0 : merkle_fuse_levels();
    if (path == kMerklePathFused && fuse == 0) fuse = kMerkleFuseChosen;
    if (fuse == 0) {
        k_merkle_leaves<<<grid_for(1ull << n), kBlock, 0, c->stream>>>(cols, k, 1ull << n, tree, P);
        for (uint32_t d = 1; d <= n; ++d) {
            const uint64_t n_out = 1ull << (n - d);
            const uint64_t *in = tree + 4 * merkle_level_offset(n, d - 1);
            uint64_t *out = tree + 4 * merkle_level_offset(n, d);
            if (n_out <= kMerkleWaveMax) k_merkle_level_wave<<<(uint32_t)n_out, 64, 0, c->stream>>>(in, out);   // latency-bound levels
            else k_merkle_level<<<grid_for(n_out), kBlock, 0, c->stream>>>(in, n_out, out);
        }
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    auto grid = [](uint64_t tiles) { return (uint32_t)(tiles < kMerkleMaxGrid ? tiles : kMerkleMaxGrid); };
    uint32_t tl = fuse < n ? fuse : n;
    k_merkle_fused<true><<<grid(1ull << (n - tl)), kBlock, (size_t)32 << tl, c->stream>>>(cols, k, tree, n, 0, tl, P);
    for (uint32_t level = tl; level < n; level += tl) {
        const uint32_t rem = n - level;
        if (rem <= kMerkleTopLog) {   // fewer nodes than a wave has lanes from here on: one workgroup, a wave per node
            k_merkle_top<<<1, kMerkleTopThreads, 0, c->stream>>>(tree, n, level, rem);
            break;
        }
        tl = fuse < rem ? fuse : rem;
        k_merkle_fused<false><<<grid(1ull << (rem - tl)), kBlock, (size_t)32 << tl, c->stream>>>(nullptr, k, tree, n, level, tl, P);
    }
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// the one entry other units use (fri.hip: a layer's column views): every level of the tree over 2^n rows of the k columns at the raw
// device pointers `cols` (host array) into `tree` (merkle_block_bytes(n) bytes), on the switch's path.  Enqueues only; no copies.
int32_t zk::merkle_build_raw(zk_ctx *c, const uint64_t *const *cols, uint32_t k, uint32_t n, uint64_t *tree) {
    if (k == 0 || k > kMerkleMaxColumns) return ZK_ERR_UNSUPPORTED;
    PoolScope ps(c);   // the pointer table goes back stream-ordered, behind the launches that read it
    const uint64_t **table = nullptr;
    ZKCHK(ps.get(scratch_bytes((size_t)k * sizeof(uint64_t *)), &table));
    for (uint32_t base = 0; base < k; base += kMerklePtrBatch) {
        MerklePtrs b = {};
        const uint32_t count = k - base < kMerklePtrBatch ? k - base : kMerklePtrBatch;
        for (uint32_t j = 0; j < count; ++j) b.p[j] = cols[base + j];
        k_merkle_put_ptrs<<<1, 64, 0, c->stream>>>(table, base, count, b);
    }
    HIPCHK(hipGetLastError());
    return merkle_build(c, table, k, n, tree, kMerklePathDefault);
}

extern "C" int32_t zk_merkle_commit(zk_ctx *c, const zk_mle *const *columns, uint32_t n_columns, zk_merkle **out) {
    if (!out) return ZK_ERR_BAD_ARG;
    ZKCHK(check_columns(c, columns, n_columns));
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)columns[0]->n_vars;
    MerkleHolder m(new (std::nothrow) zk_merkle());
    if (!m.get()) return ZK_ERR_ALLOC;
    m->ctx = c, m->n_vars = n, m->n_columns = n_columns;
    ZKCHK(m->tree.alloc(c, merkle_block_bytes(n)));
    PoolScope ps(c);
    const uint64_t *const *cols = nullptr;
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the blocks go back
    ZKCHK(put_column_ptrs(c, ps, columns, n_columns, &cols));
    ZKCHK(merkle_build(c, cols, n_columns, n, m->tree.as(), kMerklePathDefault));
    drain.armed = false;
    *out = m.release();
    return ZK_OK;
}
extern "C" int32_t zk_merkle_free(zk_merkle *m) {
    merkle_release(m);   // back to its context's pool; reuse is stream-ordered
    return ZK_OK;
}
extern "C" int32_t zk_merkle_n_vars(const zk_merkle *m, uint32_t *out) {
    if (!m || !out) return ZK_ERR_BAD_ARG;
    *out = m->n_vars;
    return ZK_OK;
}
extern "C" int32_t zk_merkle_n_columns(const zk_merkle *m, uint32_t *out) {
    if (!m || !out) return ZK_ERR_BAD_ARG;
    *out = m->n_columns;
    return ZK_OK;
}
extern "C" int32_t zk_merkle_level(zk_ctx *c, const zk_merkle *m, uint32_t level, uint8_t *out) {
    if (!c || !m || !out) return ZK_ERR_BAD_ARG;
    if (m->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (level > m->n_vars) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const uint64_t *at = m->tree.as() + 4 * merkle_level_offset(m->n_vars, level);
    HIPCHK(hipMemcpyAsync(out, at, (size_t)32 << (m->n_vars - level), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
extern "C" int32_t zk_merkle_root(zk_ctx *c, const zk_merkle *m, uint8_t out[32]) {
    if (!m) return ZK_ERR_BAD_ARG;
    return zk_merkle_level(c, m, m->n_vars, out);
}

extern "C" int32_t zk_merkle_open(zk_ctx *c, const zk_merkle *m, const zk_mle *const *columns, uint32_t n_columns, const uint64_t *indices,
                                  uint64_t n_queries, uint64_t *out_rows, uint8_t *out_paths) {
    if (!c || !m) return ZK_ERR_BAD_ARG;
    const uint32_t n = m->n_vars, k = m->n_columns;
    if (n_queries && (!indices || (n && !out_paths) || (columns && !out_rows))) return ZK_ERR_BAD_ARG;
    if (columns)
        for (uint32_t j = 0; j < n_columns; ++j)
            if (!columns[j]) return ZK_ERR_BAD_ARG;
    if (m->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (columns) {
        for (uint32_t j = 0; j < n_columns; ++j)
            if (columns[j]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
        for (uint32_t j = 0; j < n_columns; ++j)
            if (columns[j]->n_vars != n) return ZK_ERR_ARITY_MISMATCH;
        if (n_columns != k) return ZK_ERR_BAD_ARG;
    }
    if (n_queries > (1ull << kMaxVars)) return ZK_ERR_UNSUPPORTED;
    for (uint64_t q = 0; q < n_queries; ++q)
        if (indices[q] >> n) return ZK_ERR_BAD_ARG;
    if (n_queries == 0 || (n == 0 && !columns)) return ZK_OK;   // nothing to copy
    ZKCHK(use_device(c));
    PoolScope ps(c);
    const size_t path_bytes = (size_t)n_queries * n * 32, row_bytes = columns ? (size_t)n_queries * k * 32 : 0;
    uint64_t *d_idx = nullptr, *d_paths = nullptr, *d_rows = nullptr;
    const uint64_t *const *cols = nullptr;
    ZKCHK(ps.get(scratch_bytes((size_t)n_queries * 8), &d_idx));
    if (path_bytes) ZKCHK(ps.get(scratch_bytes(path_bytes), &d_paths));
    if (row_bytes) ZKCHK(ps.get(scratch_bytes(row_bytes), &d_rows));
    DrainOnExit drain(c);   // on every path: the copies read and write the caller's arrays, and the blocks go back after them
    if (columns) ZKCHK(put_column_ptrs(c, ps, columns, k, &cols));
    HIPCHK(hipMemcpyAsync(d_idx, indices, (size_t)n_queries * 8, hipMemcpyHostToDevice, c->stream));
    k_merkle_gather<<<grid_for(n_queries * (n + (columns ? k : 0))), kBlock, 0, c->stream>>>(m->tree.as(), n, d_idx, n_queries, cols, k, d_paths, d_rows);
    HIPCHK(hipGetLastError());
    if (path_bytes) HIPCHK(hipMemcpyAsync(out_paths, d_paths, path_bytes, hipMemcpyDeviceToHost, c->stream));
    if (row_bytes) HIPCHK(hipMemcpyAsync(out_rows, d_rows, row_bytes, hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

// the verifier: host only, no context.  The leaf from the row, then up the path by the bits of the index.
extern "C" int32_t zk_merkle_verify_host(int32_t field, const uint8_t root[32], uint32_t n_vars, uint32_t n_columns, uint64_t index,
                                         const uint64_t *row, const uint8_t *path, int32_t *out_ok) {
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    if (!root || !row || !out_ok || n_columns == 0 || (n_vars && !path)) return ZK_ERR_BAD_ARG;
    if (n_columns > kMerkleMaxColumns) return ZK_ERR_UNSUPPORTED;
    if (n_vars > kMaxVars || (index >> n_vars)) return ZK_ERR_BAD_ARG;
    Sponge sp;
    sp.init();
    for (uint32_t j = 0; j < n_columns; ++j) {
        const Fe e = fe_from_u64limbs(row + 4 * j);
        Fe d;
        if (!sub8(d.v, e.v, fi->P.p)) return ZK_ERR_BAD_ARG;   // not < p, as zk_fe_from_canonical refuses it
        uint64_t l[4];
        fe_to_u64limbs(fe_to_canonical(e, fi->P), l);
        uint8_t be[32];
        for (int b = 0; b < 32; ++b) be[b] = (uint8_t)(l[3 - b / 8] >> (8 * (7 - b % 8)));
        sp.update(be, 32);
    }
    uint8_t h[32];
    sp.finalize_reset(h);
    for (uint32_t d = 0; d < n_vars; ++d) {
        const uint8_t *sib = path + 32 * (size_t)d;
        const bool right = (index >> d) & 1;
        sp.update(right ? sib : h, 32);
        sp.update(right ? h : sib, 32);
        sp.finalize_reset(h);
    }
    *out_ok = memcmp(h, root, 32) == 0 ? 1 : 0;
    return ZK_OK;
}

// device time of `reps` builds of the tree over the columns (pointer table included) between two HIP events after as many untimed
// ones: path 0 = as the switch decides, 1 = the fused stages, 2 = one launch per level
extern "C" int32_t zk_bench_merkle(zk_ctx *c, const zk_mle *const *columns, uint32_t n_columns, int32_t path, int32_t reps, double *out_ms) {
    if (!out_ms || reps < 1 || path < 0 || path > 2) return ZK_ERR_BAD_ARG;
    ZKCHK(check_columns(c, columns, n_columns));
    ZKCHK(use_device(c));
    const uint32_t n = (uint32_t)columns[0]->n_vars;
    PoolBlock tree;
    ZKCHK(tree.alloc(c, merkle_block_bytes(n)));
    auto once = [&]() -> int32_t {
        PoolScope ps(c);   // every rep reuses the block of the first
        const uint64_t *const *cols = nullptr;
        ZKCHK(put_column_ptrs(c, ps, columns, n_columns, &cols));
        return merkle_build(c, cols, n_columns, n, tree.as(), path);
    };
    return timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms);
}
