// inv.hip -- host side of the batch inversion and the running products over tables (kernels in inv_kernels.cuh; no reference item,
// definition: tests/batch_inverse_ref.py).  Scratch comes from the context's pool and goes back stream-ordered.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "inv_kernels.cuh"

// Lengths up to ZK_BATCH_INV_ONE_LAUNCH_MAX (at most one chunk; 0: never) take the one-launch kernel, longer ones the three launches.
// Below a chunk both forms run the same single workgroup; the one launch saves two launch boundaries (profiles/batch_inverse.log).
static uint64_t inv_one_launch_max() {
    static const uint64_t m = env_u64("ZK_BATCH_INV_ONE_LAUNCH_MAX", kInvChunk, 0, kInvChunk);
    return m;
}
enum { kInvPathDefault = 0, kInvPathOne = 1, kInvPathThree = 2 };
// scratch sizes are rounded up to a power of two: the pool hands blocks out by exact size, so every vector length would otherwise
// open size classes of its own (the tables' and vectors' own classes are powers of two as well)
static size_t scratch_bytes(size_t bytes) {
    size_t b = 32;
    while (b < bytes) b <<= 1;
    return b;
}
// out[i] = (v[i] + shift)^-1 over n >= 1 elements, zeros to zero; out may be v.  d_count (device, one word) gets the number of
// zeros when it is not null.  Enqueues only.
static int32_t batch_inverse_device(zk_ctx *c, PoolScope &ps, const uint64_t *v, uint64_t n, const Fe &shift, uint64_t *out, uint64_t *d_count,
                                    int path = kInvPathDefault) {
    const FieldParams &P = c->fi->P;
    if (path == kInvPathOne && n > kInvChunk) return ZK_ERR_UNSUPPORTED;
    if (path == kInvPathOne || (path == kInvPathDefault && n <= inv_one_launch_max())) {
        k_inv_apply<true><<<1, kBlock, 0, c->stream>>>(v, n, shift, P, nullptr, out, d_count);
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    const uint64_t nc = (n + kInvChunk - 1) / kInvChunk;
    if (nc > 0x7fffffffull) return ZK_ERR_UNSUPPORTED;
    uint64_t *totals = nullptr, *inv = nullptr, *count = d_count;
    uint32_t *zeros = nullptr;
    ZKCHK(ps.get(scratch_bytes((size_t)nc * 32), &totals));
    ZKCHK(ps.get(scratch_bytes((size_t)nc * 32), &inv));
    ZKCHK(ps.get(scratch_bytes((size_t)nc * 4), &zeros));
    if (!count) ZKCHK(ps.get(scratch_bytes(sizeof(uint64_t)), &count));
    k_inv_chunk_products<<<(uint32_t)nc, kBlock, 0, c->stream>>>(v, n, shift, P, totals, zeros);
    k_inv_totals<<<1, kBlock, 0, c->stream>>>(totals, nc, P, inv, zeros, count);
    k_inv_apply<false><<<(uint32_t)nc, kBlock, 0, c->stream>>>(v, n, shift, P, inv, out, nullptr);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// the call with its optional count: out_zeros null -> nothing waits; else the count comes back and the stream is drained
static int32_t batch_inverse_call(zk_ctx *c, const uint64_t *v, uint64_t n, const uint64_t *shift, uint64_t *out, uint64_t *out_zeros) {
    const Fe s = shift ? fe_from_u64limbs(shift) : fe_zero();
    PoolScope ps(c);
    if (!out_zeros) return batch_inverse_device(c, ps, v, n, s, out, nullptr);
    uint64_t *d_count = nullptr;
    ZKCHK(ps.get(scratch_bytes(sizeof(uint64_t)), &d_count));
    DrainOnExit drain(c);   // the copy writes the caller's word: a failed call waits for it before returning
    ZKCHK(batch_inverse_device(c, ps, v, n, s, out, d_count));
    HIPCHK(hipMemcpyAsync(out_zeros, d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

extern "C" int32_t zk_mle_batch_inverse(zk_ctx *c, const zk_mle *t, const uint64_t *shift, zk_mle *out, uint64_t *out_zeros) {
    if (!c || !t || !out) return ZK_ERR_BAD_ARG;
    if (t->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (out->n_vars != t->n_vars) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    return batch_inverse_call(c, t->d, 1ull << t->n_vars, shift, out->d, out_zeros);
}
extern "C" int32_t zk_upoly_batch_inverse(zk_ctx *c, const zk_upoly *v, const uint64_t *shift, zk_upoly **out, uint64_t *out_zeros) {
    if (!c || !v || !out) return ZK_ERR_BAD_ARG;
    if (v->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    UpolyHolder o;
    ZKCHK(upoly_alloc(c, v->len, o.put()));
    if (v->len) {
        DrainOnExit drain(c);   // a failed call waits for what it enqueued before the result's block goes back
        ZKCHK(batch_inverse_call(c, v->d, v->len, shift, o->d, out_zeros));
        drain.armed = false;
    } else if (out_zeros) {
        *out_zeros = 0;
    }
    *out = o.release();
    return ZK_OK;
}
extern "C" int32_t zk_batch_inverse_host(zk_ctx *c, const uint64_t *in, uint64_t n, const uint64_t *shift, uint64_t *out, uint64_t *out_zeros) {
    if (!c || (n && (!in || !out))) return ZK_ERR_BAD_ARG;
    if (n > (1ull << kMaxVars)) return ZK_ERR_UNSUPPORTED;
    if (n == 0) {
        if (out_zeros) *out_zeros = 0;
        return ZK_OK;
    }
    ZKCHK(use_device(c));
    PoolBlock d;
    ZKCHK(d.alloc(c, (size_t)n * 32));
    uint64_t zeros = 0;
    DrainOnExit drain(c);   // on every path: the copies read and write the caller's arrays, and the block goes back after them
    HIPCHK(hipMemcpyAsync(d.p, in, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    ZKCHK(batch_inverse_call(c, d.as(), n, shift, d.as(), &zeros));
    HIPCHK(hipMemcpyAsync(out, d.p, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    if (out_zeros) *out_zeros = zeros;
    return ZK_OK;
}

// running product of n >= 1 elements into out (may be v); *total_at = a device pointer to the product of all (in a block of ps)
static int32_t prefix_product_device(zk_ctx *c, PoolScope &ps, const uint64_t *v, uint64_t n, bool inclusive, uint64_t *out,
                                     const uint64_t **total_at) {
    const FieldParams &P = c->fi->P;
    const uint64_t nc = (n + kPrefixChunk - 1) / kPrefixChunk;
    if (nc > 0x7fffffffull) return ZK_ERR_UNSUPPORTED;
    uint64_t *tot = nullptr;
    ZKCHK(ps.get(scratch_bytes((size_t)(nc + 1) * 32), &tot));
    k_prefix_partial<<<(uint32_t)nc, kBlock, 0, c->stream>>>(v, n, P, tot);
    k_prefix_totals<<<1, kBlock, 0, c->stream>>>(tot, nc, P);
    if (inclusive) k_prefix_apply<true><<<(uint32_t)nc, kBlock, 0, c->stream>>>(v, n, P, tot, out);
    else k_prefix_apply<false><<<(uint32_t)nc, kBlock, 0, c->stream>>>(v, n, P, tot, out);
    HIPCHK(hipGetLastError());
    *total_at = tot + 4 * nc;
    return ZK_OK;
}
extern "C" int32_t zk_mle_prefix_product(zk_ctx *c, const zk_mle *t, int32_t inclusive, zk_mle *out, uint64_t *out_total) {
    if (!c || !t || !out) return ZK_ERR_BAD_ARG;
    if (t->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (out->n_vars != t->n_vars) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    PoolScope ps(c);
    const uint64_t *total = nullptr;
    if (!out_total) return prefix_product_device(c, ps, t->d, 1ull << t->n_vars, inclusive != 0, out->d, &total);
    DrainOnExit drain(c);   // the copy writes the caller's element
    ZKCHK(prefix_product_device(c, ps, t->d, 1ull << t->n_vars, inclusive != 0, out->d, &total));
    HIPCHK(hipMemcpyAsync(out_total, total, 32, hipMemcpyDeviceToHost, c->stream));
    return drain.wait();
}

// device time of `reps` back-to-back calls between two HIP events after as many untimed ones (the kernels follow the shader clock):
// path 0 = zk_mle_batch_inverse as the switch decides, 1 = the one-launch kernel (tables of at most one chunk, else
// ZK_ERR_UNSUPPORTED), 2 = the three launches, 3 = zk_mle_prefix_product (exclusive)
extern "C" int32_t zk_bench_batch_inverse(zk_ctx *c, const zk_mle *t, zk_mle *out, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !t || !out || !out_ms || reps < 1 || path < 0 || path > 3) return ZK_ERR_BAD_ARG;
    if (t->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (out->n_vars != t->n_vars) return ZK_ERR_BAD_ARG;
    const uint64_t n = 1ull << t->n_vars;
    if (path == kInvPathOne && n > kInvChunk) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    auto once = [&]() -> int32_t {
        PoolScope ps(c);   // every rep reuses the blocks of the first
        const uint64_t *total = nullptr;
        if (path == 3) return prefix_product_device(c, ps, t->d, n, false, out->d, &total);
        return batch_inverse_device(c, ps, t->d, n, fe_zero(), out->d, nullptr, path);
    };
    return timed_span(c, reps, AfterWarm::kNoWait, reps, once, out_ms);
}
