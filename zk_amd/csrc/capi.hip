// capi.hip -- the C ABI of libzk_amd.so (include/zk_amd.h): library, context and pool, the MLE tables, the host transcript (the
// sumcheck prover and verifier: sumcheck.hip).
//
// Host logic restated from the reference (paths relative to the reference checkout):
//   sumcheck/src/lib.rs:23-29 (32-byte BE elements), transcript/src/lib.rs:16-30, polynomial/src/multilinear/evaluation_form.rs,
//   fft/src/lib.rs:4-19.  There is no CPU compute fallback: every table operation is a gfx950 kernel.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <map>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "copy_helpers.hpp"
#include "env.hpp"
#include "kernels.cuh"
#include "eval_kernels.cuh"
#include "zeta_kernels.cuh"
#include "layout_kernels.cuh"

thread_local std::string zk::g_hip_err;

struct zk_transcript {
    Sponge sp;
};
// Device blocks are recycled through a per-context free list keyed by size (tables are powers of two, so the hit
// rate is high): hipMalloc/hipFree of a 256 MiB block costs milliseconds and synchronises the device, which is more
// than a whole 2^24 fold.  All use is ordered on the context's stream, so a recycled block is safe to hand out again
// without a synchronisation.
static void pool_trim(zk_ctx *c) {   // hipFree synchronises the device, so blocks still in use by queued work are safe
    for (auto &kv : c->pool)
        for (void *q : kv.second) (void)hipFree(q);
    c->pool.clear();
    c->pool_bytes = 0;
}
// scratch that does not fit the pool's power-of-two habits still goes through here, so an allocation failure drops the cache
// and retries once instead of failing while the pool sits on idle gigabytes
int32_t zk::raw_alloc(zk_ctx *c, size_t bytes, void **out) {
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) {   // out of memory: drop the cache and retry once
        (void)hipGetLastError();
        pool_trim(c);
        e = hipMalloc(out, bytes);
    }
    if (e != hipSuccess) {
        g_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return ZK_ERR_ALLOC;
    }
    return ZK_OK;
}
int32_t zk::pool_alloc(zk_ctx *c, size_t bytes, void **out) {
    if (bytes == 0) bytes = 32;
    auto it = c->pool.find(bytes);
    if (it != c->pool.end() && !it->second.empty()) {
        *out = it->second.back();
        it->second.pop_back();
        c->pool_bytes -= bytes;
        return ZK_OK;
    }
    return raw_alloc(c, bytes, out);
}
// Takes a block back under the size it was allocated with: the pool hands it out again by exact size, so a free that names
// another size would corrupt memory.  Host code therefore never calls this with a size written at the call site -- every block
// has an owner (PoolBlock, PoolScope, or a handle behind Scoped below) that recorded the size when it allocated.
void zk::pool_free(zk_ctx *c, void *ptr, size_t bytes) {
    if (!ptr) return;
    if (bytes == 0) bytes = 32;
    try {   // runs in the owners' destructors, on unwinding paths too: no exception leaves it
        c->pool[bytes].push_back(ptr);
    } catch (...) {   // no host memory for the free list: the block goes back to the device instead (hipFree waits for its users)
        (void)hipFree(ptr);
        return;
    }
    c->pool_bytes += bytes;
    // cap: idle blocks never hold more than half of what the device has left (other contexts, other libraries and this
    // library's few raw hipMallocs must not fail while gigabytes sit here).  Checked only past 1 GiB: hipMemGetInfo is slow.
    // (pool_alloc lowers pool_bytes without touching pool_checked: compare before subtracting, the difference is unsigned)
    if (c->pool_bytes > ((size_t)1 << 30) && c->pool_bytes > c->pool_checked && c->pool_bytes - c->pool_checked > ((size_t)1 << 30)) {
        size_t fr = 0, tot = 0;
        c->pool_checked = c->pool_bytes;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && c->pool_bytes > fr / 2) {
            pool_trim(c);
            c->pool_checked = 0;
        }
    }
}
// ------------------------------------------------------------------------------------------------------------
// library
// ------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_abi_version(void) { return ZK_AMD_ABI_VERSION; }

extern "C" const char *zk_strerror(int32_t s) {
    switch (s) {
        case ZK_OK: return "ok";
        case ZK_ERR_EVAL_LEN: return "evaluation vec len should equal 2^n_vars";
        case ZK_ERR_EVAL_ARITY: return "evaluate must assign to all variables";
        case ZK_ERR_EMPTY_PRODUCT: return "cannot create product polynomial from empty polynomials";
        case ZK_ERR_ARITY_MISMATCH:
            return "cannot create product polynomial from polynomial that don't share the same number of variables";
        case ZK_ERR_PANIC_INDEX: return "reference panics: index arithmetic underflow (initial_var / assignments out of range)";
        case ZK_ERR_FFT_NOT_POW2: return "values must be a power of 2";
        case ZK_ERR_FFT_NO_ROOT: return "reference panics: get_root_of_unity returned None";
        case ZK_ERR_VERIFY_ROUNDS: return "invalid proof: require 1 round poly for each variable in poly";
        case ZK_ERR_VERIFY_SUM: return "verifier check failed: claimed_sum != p(0) + p(1)";
        case ZK_ERR_COEFF_RANGE: return "coefficient map represents more than specificed number of variables";
        case ZK_ERR_PANIC_INVERSE: return "reference panics: (x_i - x_j).inverse().unwrap() on a repeated x (interpolate_xy)";
        case ZK_ERR_EVAL_ASSIGNMENT: return "evaluate requires an assignment for every variable";
        case ZK_ERR_SELECTOR_LEN: return "the selector array len should be the same as the number of variables";
        case ZK_ERR_SELECTOR_SINGLE: return "only select single variable, cannot get indexes for constant or multiple variables";
        case ZK_ERR_BAD_ARG: return "bad argument";
        case ZK_ERR_BAD_FIELD: return "unknown field id";
        case ZK_ERR_NO_DEVICE: return "no usable gfx950 device (libzk_amd has no CPU fallback)";
        case ZK_ERR_HIP: return "HIP runtime error (see zk_last_hip_error)";
        case ZK_ERR_ALLOC: return "allocation failed";
        case ZK_ERR_UNSUPPORTED: return "unsupported configuration";
        case ZK_ERR_CONTEXT_MISMATCH: return "handle belongs to a different context";
        case ZK_ERR_GKR_REJECT: return "gkr verifier check failed: layer wiring / input claim mismatch";
        case ZK_ERR_COMM: return "collective failed (see zk_last_hip_error)";
        default: return "unknown status";
    }
}
extern "C" const char *zk_last_hip_error(void) { return g_hip_err.c_str(); }

extern "C" int32_t zk_device_count(int32_t *out) {
    if (!out) return ZK_ERR_BAD_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// field helpers (host)
// ------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_field_modulus(int32_t field, uint64_t out[4]) {
    const uint64_t *m = field_modulus_limbs(field);
    if (!m || !out) return m ? ZK_ERR_BAD_ARG : ZK_ERR_BAD_FIELD;
    memcpy(out, m, 32);
    return ZK_OK;
}
extern "C" int32_t zk_field_two_adicity(int32_t field, int32_t *out) {
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    if (!out) return ZK_ERR_BAD_ARG;
    *out = (int32_t)fi->two_adicity;
    return ZK_OK;
}
// F::get_root_of_unity(2^log_n) (fft/src/lib.rs:6): None -> ZK_ERR_FFT_NO_ROOT
extern "C" int32_t zk_field_root_of_unity(int32_t field, uint64_t log_n, uint64_t out[4]) {
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    if (!out) return ZK_ERR_BAD_ARG;
    Fe w;
    if (log_n > 64 || !field_root_of_unity(*fi, (uint32_t)log_n, w)) return ZK_ERR_FFT_NO_ROOT;
    fe_to_u64limbs(w, out);
    return ZK_OK;
}
extern "C" int32_t zk_fe_from_u64(int32_t field, uint64_t v, uint64_t out[4]) {
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    uint64_t l[4] = {v, 0, 0, 0};
    fe_to_u64limbs(fe_from_canonical(fe_from_u64limbs(l), fi->P), out);
    return ZK_OK;
}
extern "C" int32_t zk_fe_from_canonical(int32_t field, const uint64_t limbs[4], uint64_t out[4]) {
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    Fe c = fe_from_u64limbs(limbs), d;
    if (!sub8(d.v, c.v, fi->P.p)) return ZK_ERR_BAD_ARG;   // not < p
    fe_to_u64limbs(fe_from_canonical(c, fi->P), out);
    return ZK_OK;
}
extern "C" int32_t zk_fe_to_canonical(int32_t field, const uint64_t a[4], uint64_t out[4]) {
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    fe_to_u64limbs(fe_to_canonical(fe_from_u64limbs(a), fi->P), out);
    return ZK_OK;
}
extern "C" int32_t zk_fe_from_be_bytes_mod_order(int32_t field, const uint8_t *bytes, size_t len, uint64_t out[4]) {
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    fe_to_u64limbs(fe_from_be_bytes_mod_order(bytes, len, fi->P), out);
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------------------
// the device side of a new context; on a failure the caller tears down whatever exists so far
static int32_t ctx_init_device(zk_ctx *c) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    HIPCHK(hipMalloc(&c->d_partials, (size_t)kMaxGrid * kMaxSums * 32));
    HIPCHK(hipMalloc(&c->d_sums, (size_t)kMaxSums * 32 * 3));
    // completion word + result staging are POLLED by the host while the kernel that writes them is still running: ask for
    // coherent (fine-grained) mapped memory explicitly instead of relying on HIP_HOST_COHERENT's default
    HIPCHK(hipHostMalloc(&c->h_pinned, (size_t)kMaxSums * 32 * 3, kPolledHostFlags));
    HIPCHK(hipHostMalloc((void **)&c->h_flag, 64 * kMaxBatch, kPolledHostFlags));   // one 64-byte line per proof of a batch (slot 0: every other call)
    memset(c->h_flag, 0, 64 * kMaxBatch);
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    return ZK_OK;
}
// everything a context holds, whether it was built completely (zk_ctx_destroy) or not (a failed zk_ctx_create)
static void ctx_teardown(zk_ctx *c) {
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->stream);
    for (auto &kv : c->twiddles) (void)hipFree(kv.second);
    for (auto &kv : c->lagrange_w) (void)hipFree(kv.second);
    for (auto &kv : c->ntt_plans) {
        (void)hipFree((void *)kv.second.w_lo);
        (void)hipFree((void *)kv.second.w_hi);
        for (int p = 0; p < 4; ++p)
            if (kv.second.w_full[p]) (void)hipFree((void *)kv.second.w_full[p]);
    }
    pool_trim(c);
    (void)hipFree(c->d_partials);
    (void)hipFree(c->d_sums);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->h_flag) (void)hipHostFree(c->h_flag);
    if (c->h_results) (void)hipHostFree(c->h_results);
    for (int b = 0; b < 2; ++b) {
        if (c->h_absorb[b]) (void)hipHostFree(c->h_absorb[b]);
        if (c->ev_absorb[b]) (void)hipEventDestroy(c->ev_absorb[b]);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}
extern "C" int32_t zk_ctx_create(int32_t field, int32_t device, zk_ctx **out) {
    if (!out) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return ZK_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ZK_ERR_NO_DEVICE;
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) return ZK_ERR_NO_DEVICE;   // gfx950 code object only
    zk_ctx *c = new (std::nothrow) zk_ctx();
    if (!c) return ZK_ERR_ALLOC;
    c->field = field;
    c->device = device;
    c->fi = fi;
    c->own_stream = c->stream = nullptr;
    c->ev0 = c->ev1 = nullptr;
    c->d_partials = c->d_sums = c->h_pinned = nullptr;
    c->h_flag = nullptr;
    c->flag_seq = 0;
    c->h_results = nullptr;
    c->h_results_bytes = 0;
    c->pool_bytes = c->pool_checked = 0;
    c->inv2 = fe_inverse(fe_from_u32(2, fi->P), fi->P);
    c->pipe_consts.inv2p = mul29_prepare(c->inv2, fi->P);
    {
        Fe v = {{1, 0, 0, 0, 0, 0, 0, 0}};   // the integer 1; doubled 266 times modulo p (fe_add works on any residues < p)
        for (int i = 0; i < 266; ++i) v = fe_add(v, v, fi->P);
        split29(v.v, c->pipe_consts.k266.l);
    }
    c->d_dbg = nullptr;
    c->dbg_launch = 0;
    c->h_absorb[0] = c->h_absorb[1] = nullptr;
    c->h_absorb_bytes = 0;
    c->ev_absorb[0] = c->ev_absorb[1] = nullptr;
    const int32_t rc = ctx_init_device(c);
    if (rc != ZK_OK) {
        ctx_teardown(c);
        return rc;
    }
    *out = c;
    return ZK_OK;
}
extern "C" int32_t zk_ctx_destroy(zk_ctx *c) {
    if (!c) return ZK_OK;
    ctx_teardown(c);
    return ZK_OK;
}
extern "C" int32_t zk_ctx_synchronize(zk_ctx *c) {
    if (!c) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
extern "C" int32_t zk_ctx_set_stream(zk_ctx *c, void *s) {
    if (!c) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t)s;   // NULL is the legacy default stream (what torch uses unless told otherwise)
    return ZK_OK;
}
extern "C" int32_t zk_ctx_use_own_stream(zk_ctx *c) {
    if (!c) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = c->own_stream;
    return ZK_OK;
}
extern "C" int32_t zk_ctx_trim(zk_ctx *c) {
    if (!c) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    pool_trim(c);
    c->pool_checked = 0;
    return ZK_OK;
}
extern "C" int32_t zk_ctx_field(const zk_ctx *c, int32_t *out) {
    if (!c || !out) return ZK_ERR_BAD_ARG;
    *out = c->field;
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// MultiLinearPolynomial
// ------------------------------------------------------------------------------------------------------------
int32_t zk::mle_alloc(zk_ctx *c, uint64_t n_vars, zk_mle **out) {
    if (n_vars > kMaxVars) return ZK_ERR_UNSUPPORTED;
    zk_mle *t = new (std::nothrow) zk_mle();
    if (!t) return ZK_ERR_ALLOC;
    t->ctx = c;
    t->n_vars = n_vars;
    PoolBlock blk;
    const int32_t rc = blk.alloc(c, mle_block_bytes(n_vars));
    if (rc != ZK_OK) {
        delete t;
        return rc;
    }
    t->d = static_cast<uint64_t *>(blk.release());   // the handle owns the block from here on (mle_release)
    *out = t;
    return ZK_OK;
}
void zk::mle_release(zk_mle *t) {
    if (!t) return;
    pool_free(t->ctx, t->d, mle_block_bytes(t->n_vars));
    delete t;
}
extern "C" int32_t zk_mle_alloc(zk_ctx *c, uint64_t n_vars, zk_mle **out) {
    if (!c || !out) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    return mle_alloc(c, n_vars, out);
}
extern "C" int32_t zk_mle_upload(zk_ctx *c, uint64_t n_vars, const uint64_t *evals, uint64_t len, zk_mle **out) {
    if (!c || !out || (!evals && len)) return ZK_ERR_BAD_ARG;
    if (n_vars >= 64 || len != (1ull << n_vars)) return ZK_ERR_EVAL_LEN;   // evaluation_form.rs:19-21
    ZKCHK(use_device(c));
    MleHolder t;
    ZKCHK(mle_alloc(c, n_vars, t.put()));
    hipError_t e = hipMemcpyAsync(t->d, evals, (size_t)len * 32, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        g_hip_err = std::string("upload: ") + hipGetErrorString(e);
        return ZK_ERR_HIP;
    }
    *out = t.release();
    return ZK_OK;
}
extern "C" int32_t zk_mle_fill_random(zk_ctx *c, zk_mle *t, uint64_t seed, uint64_t first) {
    if (!c || !t) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    const uint64_t n = 1ull << t->n_vars;
    k_fill_random<<<grid_for(n), kBlock, 0, c->stream>>>(t->d, n, seed, first, c->fi->P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
extern "C" int32_t zk_mle_clone(zk_ctx *c, const zk_mle *t, zk_mle **out) {
    if (!c || !t || !out) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    MleHolder o;
    ZKCHK(mle_alloc(c, t->n_vars, o.put()));
    HIPCHK(hipMemcpyAsync(o->d, t->d, (size_t)32 << t->n_vars, hipMemcpyDeviceToDevice, c->stream));
    *out = o.release();
    return ZK_OK;
}
extern "C" int32_t zk_mle_free(zk_ctx *c, zk_mle *t) {
    if (!t) return ZK_OK;
    if (!c || t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    mle_release(t);   // back to the context's pool; reuse is stream-ordered
    return ZK_OK;
}
extern "C" int32_t zk_mle_n_vars(const zk_mle *t, uint64_t *out) {
    if (!t || !out) return ZK_ERR_BAD_ARG;
    *out = t->n_vars;
    return ZK_OK;
}
extern "C" int32_t zk_mle_download(zk_ctx *c, const zk_mle *t, uint64_t *out) {
    if (!c || !t || !out) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    HIPCHK(hipMemcpyAsync(out, t->d, (size_t)32 << t->n_vars, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
// #[derive(PartialEq)] (evaluation_form.rs:4): same n_vars and the same evaluations.  Elements are canonical (< p), so
// equality of representatives is equality in F_p.
extern "C" int32_t zk_mle_equal(zk_ctx *c, const zk_mle *a, const zk_mle *b, int32_t *out) {
    if (!c || !a || !b || !out) return ZK_ERR_BAD_ARG;
    if (a->ctx != c || b->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (a->n_vars != b->n_vars) {
        *out = 0;
        return ZK_OK;
    }
    if (a->d == b->d) {
        *out = 1;
        return ZK_OK;
    }
    ZKCHK(use_device(c));
    uint32_t *d_flag = reinterpret_cast<uint32_t *>(c->d_sums);
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, c->stream));
    const uint64_t n16 = (uint64_t)2 << a->n_vars;
    k_compare<<<grid_for(n16), kBlock, 0, c->stream>>>(reinterpret_cast<const uint4 *>(a->d), reinterpret_cast<const uint4 *>(b->d), n16, d_flag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_pinned, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = *reinterpret_cast<uint32_t *>(c->h_pinned) == 0 ? 1 : 0;
    return ZK_OK;
}
extern "C" int32_t zk_mle_device_ptr(const zk_mle *t, void **out) {
    if (!t || !out) return ZK_ERR_BAD_ARG;
    *out = t->d;
    return ZK_OK;
}

// one assignment of partial_evaluate (evaluation_form.rs:54-72) as a kernel launch
static int32_t launch_fold(zk_ctx *c, const uint64_t *in, uint64_t *out, uint64_t m, uint64_t initial_var, const Fe &r) {
    const uint64_t pairs = 1ull << (m - 1);
    const uint32_t pos = (uint32_t)(m - 1 - initial_var);
    if (initial_var == 0 && pairs >= 64) {   // the sumcheck fold: lane-pair coalesced, nontemporal streaming kernel
        uint64_t g = pairs / kBlock;           // one 64-element run per wave
        if (g > 2 * kMaxGridStream) g = 2 * kMaxGridStream;
        k_fold_msb<<<(uint32_t)(g ? g : 1), kBlock, 0, c->stream>>>(in, out, pairs, c->fi->P, mul29_prepare(r, c->fi->P));
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    if (pos >= 6 && in != out) {   // any other variable whose pair partner is >= 64 elements away: the same run access, block by block
        uint64_t g = pairs / kBlock;
        if (g > 2 * kMaxGridStream) g = 2 * kMaxGridStream;
        k_fold_run<<<(uint32_t)(g ? g : 1), kBlock, 0, c->stream>>>(in, out, pairs, pos, c->fi->P, mul29_prepare(r, c->fi->P));
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    if (pos < 6 && pairs >= 64 && in != out) {   // partner inside the wave's 128-element run: one in-wave exchange (k_fold_low)
        uint64_t g = pairs / kBlock;
        if (g > 2 * kMaxGridStream) g = 2 * kMaxGridStream;
        k_fold_low<<<(uint32_t)(g ? g : 1), kBlock, 0, c->stream>>>(in, out, pairs, pos, c->fi->P, mul29_prepare(r, c->fi->P));
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    uint64_t g = (pairs + kBlock - 1) / kBlock;
    if (g > kMaxGridStream) g = kMaxGridStream;
    k_fold<<<(uint32_t)(g ? g : 1), kBlock, 0, c->stream>>>(in, out, pairs, pos, c->fi->P, mul29_prepare(r, c->fi->P));
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// the reference's panics (u8 / usize underflow at evaluation_form.rs:55,75 and pairing_index.rs:3,6) as a status
static int32_t check_partial_args(uint64_t n_vars, uint64_t initial_var, uint64_t n_assign) {
    if (n_assign > n_vars) return ZK_ERR_PANIC_INDEX;
    for (uint64_t i = 0; i < n_assign; ++i) {
        const uint64_t nv = n_vars - i;
        if (nv == 0 || initial_var > nv - 1) return ZK_ERR_PANIC_INDEX;
    }
    return ZK_OK;
}

extern "C" int32_t zk_mle_partial_evaluate(zk_ctx *c, const zk_mle *t, uint64_t initial_var, const uint64_t *assignments,
                                           uint64_t n_assign, zk_mle **out) {
    if (!c || !t || !out || (!assignments && n_assign)) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(check_partial_args(t->n_vars, initial_var, n_assign));
    ZKCHK(use_device(c));
    if (n_assign == 0) return zk_mle_clone(c, t, out);
    MleHolder res, tmp[2];
    ZKCHK(mle_alloc(c, t->n_vars - n_assign, res.put()));
    if (n_assign >= 2) ZKCHK(mle_alloc(c, t->n_vars - 1, tmp[0].put()));
    if (n_assign >= 3) ZKCHK(mle_alloc(c, t->n_vars - 2, tmp[1].put()));
    const uint64_t *src = t->d;
    for (uint64_t i = 0; i < n_assign; ++i) {
        uint64_t *dst = (i == n_assign - 1) ? res->d : tmp[i & 1]->d;
        ZKCHK(launch_fold(c, src, dst, t->n_vars - i, initial_var, fe_from_u64limbs(assignments + 4 * i)));
        src = dst;
    }
    *out = res.release();
    return ZK_OK;
}

extern "C" int32_t zk_mle_fold_into(zk_ctx *c, const zk_mle *t, const uint64_t r[4], zk_mle *out) {
    if (!c || !t || !r || !out) return ZK_ERR_BAD_ARG;
    if (t->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (t->n_vars == 0) return ZK_ERR_PANIC_INDEX;
    if (out->n_vars != t->n_vars - 1) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    return launch_fold(c, t->d, out->d, t->n_vars, 0, fe_from_u64limbs(r));
}

// evaluate (evaluation_form.rs:83-89): MSB folds -- the first out of place into scratch, the next ones in place there,
// and the last <= kEvalTailVars variables in one single-workgroup launch (k_evaluate_tail)
// flag_seq != 0: d_out_elem is pinned host memory and the kernel that writes it also stores flag_seq into c->h_flag (host_flag_wait)
int32_t zk::evaluate_device(zk_ctx *c, const zk_mle *t, const uint64_t *point, uint64_t *d_out_elem, uint32_t flag_seq) {
    const uint64_t n = t->n_vars;
    if (n == 0) {
        HIPCHK(hipMemcpyAsync(d_out_elem, t->d, 32, hipMemcpyDeviceToDevice, c->stream));
        return ZK_OK;
    }
    const FieldParams &P = c->fi->P;
    // bulk: the LOW variables first, 8-12 per launch (k_eval_low, one workgroup per output element).  With 8..12 variables left one
    // workgroup finishes and writes the result; with more, a launch leaves 8 for that last one when 8..12 low variables get
    // there, otherwise it takes 12; fewer than 8 left over go to k_evaluate_tail.
    PoolBlock scratch[2];   // back to the pool when the call returns: stream-ordered reuse
    const uint64_t *src = t->d;
    uint64_t cur = n;   // variables left
    static const bool bulk_low = !env_flag("ZK_EVAL_FOLDS");   // ZK_EVAL_FOLDS=1: the variable-by-variable path (A/B, tests)
    // tables of at least this many variables take the streaming kernel (k_eval_stream: up to 15 variables per launch, half an
    // element per lane, carry-free column sums); smaller ones are launch latency and keep k_eval_low.  ZK_EVAL_STREAM_MIN overrides.
    static const uint64_t stream_min = env_u64("ZK_EVAL_STREAM_MIN", 21, 0, 1000);   // above kMaxVars: never
    for (int pass = 0; bulk_low && cur >= 8; ++pass) {
        // the streaming launch leaves 9 variables (512 workgroups), 8 at 21 variables: every workgroup spends ~2600 instructions per
        // wave on its weight tables before the first product, so at 2^21 elements half as many workgroups with twice the rows win
        // (device time 31.2 -> 29.1 us; 10 left: 54 us -- profiles/r04_evaluate_stream_grid_ab.log).  ZK_EVAL_STREAM_LEAVE overrides.
        static const uint64_t leave_env = env_u64("ZK_EVAL_STREAM_LEAVE", 0, 7, kEvalHighMax);   // 0 = not set
        const uint64_t stream_leave = leave_env ? leave_env : (cur <= 21 ? (uint64_t)8 : (uint64_t)9);
        const bool stream = cur >= stream_min && cur >= (uint64_t)kEvalStreamMin + stream_leave;
        uint64_t L = cur <= (uint64_t)kEvalLowMax ? cur : cur - 8;
        if (L > (uint64_t)kEvalLowMax) L = kEvalLowMax;
        if (L < (uint64_t)kEvalLowMin) L = kEvalLowMin;   // cur >= 13 here
        if (stream) L = cur - stream_leave < (uint64_t)kEvalStreamMax ? cur - stream_leave : (uint64_t)kEvalStreamMax;
        const uint64_t n_out = 1ull << (cur - L);
        uint64_t *dst = d_out_elem;
        if (L != cur) {
            const int b = pass & 1;
            if (!scratch[b] || scratch[b].bytes < n_out * 32) ZKCHK(scratch[b].alloc(c, (size_t)n_out * 32));
            dst = scratch[b].as();
        }
        // when at most kEvalHighMax variables remain after this launch its workgroups weight their outputs with eq(point_high, g)
        // (common.cuh eval_high_weight) and what is left is a plain sum of the 2^H outputs (k_eval_sum) instead of another bulk launch
        const uint64_t H = cur - L;
        EvalHighPoint ph = {};
        static const int weight_mode = (int)env_u64("ZK_EVAL_WEIGHT", 3, 0, 3);   // A/B: bit 0 = k_eval_low, bit 1 = k_eval_stream
        if (H >= 1 && H <= (uint64_t)kEvalHighMax && (weight_mode & (stream ? 2 : 1))) {
            ph.n = (uint32_t)H;
            for (uint64_t p = 0; p < H; ++p) {
                const Fe r = fe_from_u64limbs(point + 4 * (H - 1 - p));   // bit p of the output index <-> variable H-1-p of the point
                for (int i = 0; i < 8; ++i) ph.r[p][i] = r.v[i];
            }
        }
        if (stream) {
            EvalStreamPoint sp = {};
            for (uint64_t p = 0; p < L; ++p) {
                const Fe r = fe_from_u64limbs(point + 4 * (cur - 1 - p));   // index bit p <-> variable cur-1-p (variable 0 is the MSB)
                for (int i = 0; i < 8; ++i) sp.r[p][i] = r.v[i];
            }
            const Fe two128 = {{0, 0, 0, 0, 1, 0, 0, 0}};
            const Fe c128 = fe_from_canonical(two128, P);
            for (int i = 0; i < 8; ++i) sp.c128[i] = c128.v[i];
            k_eval_stream<<<(uint32_t)n_out, kEvalStreamThreads, 0, c->stream>>>(src, dst, (uint32_t)L, sp, P, ph);
        } else {
            EvalLowPoint pt = {};
            for (uint64_t p = 0; p < L; ++p) {
                const Fe r = fe_from_u64limbs(point + 4 * (cur - 1 - p));   // index bit p <-> variable cur-1-p (variable 0 is the MSB)
                for (int i = 0; i < 8; ++i) pt.r[p][i] = r.v[i];
            }
            k_eval_low<<<(uint32_t)n_out, kBlock, 0, c->stream>>>(src, dst, (uint32_t)L, pt, P, (flag_seq && L == cur) ? c->h_flag : nullptr, flag_seq, ph);
        }
        HIPCHK(hipGetLastError());
        src = dst;
        cur -= L;
        if (ph.n) {   // the outputs carry their weights: the result is their sum
            k_eval_sum<<<1, kBlock, 0, c->stream>>>(src, (uint32_t)n_out, P, d_out_elem, flag_seq ? c->h_flag : nullptr, flag_seq);
            HIPCHK(hipGetLastError());
            cur = 0;
            break;
        }
    }
    if (bulk_low && cur == 0) return ZK_OK;   // the last k_eval_low has written the result
    const uint64_t tail_vars = cur < (uint64_t)kEvalTailVars ? cur : (uint64_t)kEvalTailVars;
    const uint64_t big = cur - tail_vars;                    // folds done as full launches (ZK_EVAL_FOLDS only)
    PoolBlock fold_block;
    if (big) ZKCHK(fold_block.alloc(c, (size_t)32 << (cur - 1)));
    uint64_t *const fold_scratch = fold_block.as();
    for (uint64_t i = 0; i < big;) {
        const uint64_t left = big - i, m = cur - i;
        if (left >= 2) {   // three (or two) variables per launch
            const int v = left >= 3 ? 3 : 2;
            FoldChallenges ch = {};
            for (int u = 0; u < v; ++u) ch.r[u] = mul29_prepare(fe_from_u64limbs(point + 4 * (i + u)), P);
            const uint64_t n_out = 1ull << (m - v);
            if (v == 3) k_fold_multi<3><<<grid_for(n_out), kBlock, 0, c->stream>>>(src, fold_scratch, n_out, P, ch);
            else k_fold_multi<2><<<grid_for(n_out), kBlock, 0, c->stream>>>(src, fold_scratch, n_out, P, ch);
            HIPCHK(hipGetLastError());
            i += v;
        } else {
            ZKCHK(launch_fold(c, src, fold_scratch, m, 0, fe_from_u64limbs(point + 4 * (i))));
            i += 1;
        }
        src = fold_scratch;
    }
    // the remaining assignments travel in the kernel arguments: no staging buffer, no synchronisation
    EvalTailChallenges chs = {};
    for (uint64_t v = 0; v < tail_vars; ++v) {
        const Mul29 r = mul29_prepare(fe_from_u64limbs(point + 4 * (big + v)), P);
        for (int i = 0; i < 9; ++i) chs.w[v][i] = r.l[i];
    }
    const size_t lds = (size_t)32 << (tail_vars - 1);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_evaluate_tail), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_evaluate_tail<<<1, kEvalTailThreads, lds, c->stream>>>(src, (uint32_t)tail_vars, chs, P, d_out_elem, flag_seq ? c->h_flag : nullptr, flag_seq);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
extern "C" int32_t zk_mle_evaluate(zk_ctx *c, const zk_mle *t, const uint64_t *point, uint64_t n_point, uint64_t out[4]) {
    if (!c || !t || !out || (!point && n_point)) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (n_point != t->n_vars) return ZK_ERR_EVAL_ARITY;   // evaluation_form.rs:84-86
    ZKCHK(use_device(c));
    static const bool host_dbg = env_flag("ZK_HOST_DEBUG");
    const auto t_enter = std::chrono::steady_clock::now();
    if (t->n_vars == 0) {
        ZKCHK(evaluate_device(c, t, point, c->d_sums));
        HIPCHK(hipMemcpyAsync(c->h_pinned, c->d_sums, 32, hipMemcpyDeviceToHost, c->stream));
    } else {
        // the last kernel stores the 32-byte result straight into the pinned host buffer (mapped into the device's address space):
        // a device-to-host copy of 32 bytes is a blit launch of its own (4-5 us on the stream)
        const uint32_t seq = next_flag_seq(c);
        ZKCHK(evaluate_device(c, t, point, c->h_pinned, seq));
        const auto t_enq0 = std::chrono::steady_clock::now();
        ZKCHK(host_flag_wait(c, seq));   // the completion word the last kernel stores next to the result
        if (host_dbg) {
            const auto t_done = std::chrono::steady_clock::now();
            fprintf(stderr, "[host] evaluate n=%llu: enqueue %.1f us, wait %.1f us\n", (unsigned long long)t->n_vars,
                    std::chrono::duration<double, std::micro>(t_enq0 - t_enter).count(),
                    std::chrono::duration<double, std::micro>(t_done - t_enq0).count());
        }
        memcpy(out, c->h_pinned, 32);
        return ZK_OK;
    }
    const auto t_enq = std::chrono::steady_clock::now();
    HIPCHK(stream_wait(c->stream));
    if (host_dbg) {
        const auto t_done = std::chrono::steady_clock::now();
        fprintf(stderr, "[host] evaluate n=%llu: enqueue %.1f us, wait %.1f us\n", (unsigned long long)t->n_vars,
                std::chrono::duration<double, std::micro>(t_enq - t_enter).count(),
                std::chrono::duration<double, std::micro>(t_done - t_enq).count());
    }
    memcpy(out, c->h_pinned, 32);
    return ZK_OK;
}

extern "C" int32_t zk_mle_to_bytes(zk_ctx *c, const zk_mle *t, uint8_t *out) {
    if (!c || !t || !out) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    // device serialiser -> pinned staging (two buffers, the copy of chunk i + 1 under the host's copy-out of chunk i) -> caller
    size_t off = 0;
    const zk_mle *one[1] = {t};
    CopyHelpers helpers((size_t)32 << t->n_vars);
    return stream_table_bytes(c, one, 1, [&](const uint8_t *p, size_t bytes) {
        helpers.copy(out + off, p, bytes);
        off += bytes;
    });
}

extern "C" int32_t zk_mle_partial_evaluate_host(zk_ctx *c, uint64_t n_vars, const uint64_t *evals, uint64_t len,
                                                uint64_t initial_var, const uint64_t *assignments, uint64_t n_assign,
                                                uint64_t *out_evals) {
    if (!out_evals) return ZK_ERR_BAD_ARG;
    MleHolder t, o;
    ZKCHK(zk_mle_upload(c, n_vars, evals, len, t.put()));
    ZKCHK(zk_mle_partial_evaluate(c, t.get(), initial_var, assignments, n_assign, o.put()));
    return zk_mle_download(c, o.get(), out_evals);
}

// ---- sharding by index mod world (layout_kernels.cuh): rank g holds {idx : idx mod world == g}, local index idx / world --------
static bool shard_world_ok(uint64_t n_vars, uint32_t world) {
    return world != 0 && (world & (world - 1)) == 0 && world <= 65536 && n_vars <= kMaxVars && (uint64_t)world <= (1ull << n_vars);
}
uint32_t zk::log2_world(uint32_t world) {
    uint32_t lw = 0;
    while ((1u << lw) < world) ++lw;
    return lw;
}
// where the kernels find shard g: in the kernel arguments (world <= kShardArgPtrs) or in a device pointer table from the pool,
// staged from the host (the call then waits for the stream once).  d_table (if set) goes back to the pool with its owner, after the launch.
static int32_t shard_src(zk_ctx *c, const std::vector<uint64_t *> &ptrs, ShardSrc &s, PoolBlock &d_table) {
    s = {};
    if (ptrs.size() <= (size_t)kShardArgPtrs) {
        for (size_t g = 0; g < ptrs.size(); ++g) s.ptrs.p[g] = reinterpret_cast<uint4 *>(ptrs[g]);
        return ZK_OK;
    }
    const size_t bytes = ptrs.size() * sizeof(void *);
    ZKCHK(d_table.alloc(c, bytes));
    if (hipMemcpyAsync(d_table.p, ptrs.data(), bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        g_hip_err = "shard pointer table: " + std::string(hipGetErrorString(hipGetLastError()));
        d_table.reset();
        return ZK_ERR_HIP;
    }
    s.table = reinterpret_cast<uint4 *const *>(d_table.p);
    return ZK_OK;
}
// natural table of 2^n_vars elements <-> 2^log_w shards of 2^(n_vars - log_w) (split: natural -> shards)
static int32_t launch_shard_layout(zk_ctx *c, bool split, uint64_t *natural, const ShardSrc &shards, uint32_t log_w, uint64_t n_vars) {
    const uint64_t world = 1ull << log_w, m = 1ull << (n_vars - log_w), n_slots = 2ull << n_vars;
    uint4 *nat = reinterpret_cast<uint4 *>(natural);
    if (world >= (uint64_t)kTileG && m >= (uint64_t)kTileJ) {
        const uint64_t tiles = (world / kTileG) * (m / kTileJ);
        const uint32_t g = (uint32_t)(tiles < kMaxGridStream ? tiles : kMaxGridStream);
        if (split) k_shard_split_tiled<<<g, kBlock, 0, c->stream>>>(nat, shards, log_w, m);
        else k_shard_interleave_tiled<<<g, kBlock, 0, c->stream>>>(shards, nat, log_w, m);
    } else {
        const uint64_t per_block = (uint64_t)kBlock * kShardUnroll;
        uint64_t g = (n_slots + per_block - 1) / per_block;
        if (g > kMaxGridStream) g = kMaxGridStream;
        if (split) k_shard_split_direct<<<(uint32_t)g, kBlock, 0, c->stream>>>(nat, shards, log_w, n_slots);
        else k_shard_interleave_direct<<<(uint32_t)g, kBlock, 0, c->stream>>>(shards, nat, log_w, n_slots);
    }
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// interleave of `world` shards of 2^m elements each, given as separate tables (ptrs) or one rank-major buffer (major)
int32_t zk::shard_interleave(zk_ctx *c, const std::vector<uint64_t *> &ptrs, uint64_t *major, uint32_t world, uint64_t m, zk_mle **out) {
    const uint32_t lw = log2_world(world);
    if (m + lw > kMaxVars) return ZK_ERR_UNSUPPORTED;
    MleHolder o;
    ZKCHK(mle_alloc(c, m + lw, o.put()));
    ShardSrc src = {};
    PoolBlock d_table;   // stream-ordered reuse
    if (major) src.major = reinterpret_cast<uint4 *>(major);
    else ZKCHK(shard_src(c, ptrs, src, d_table));
    ZKCHK(launch_shard_layout(c, false, o->d, src, lw, m + lw));
    *out = o.release();
    return ZK_OK;
}
extern "C" int32_t zk_mle_split(zk_ctx *c, const zk_mle *t, uint32_t world, zk_mle **out) {
    if (!c || !t || !out) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (!shard_world_ok(t->n_vars, world)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const uint32_t lw = log2_world(world);
    // on an early return the shards made so far go back (stream-ordered: nothing queued can still write them unsafely)
    std::vector<MleHolder> shards(world);
    std::vector<uint64_t *> ptrs(world, nullptr);
    for (uint32_t g = 0; g < world; ++g) {
        ZKCHK(mle_alloc(c, t->n_vars - lw, shards[g].put()));
        ptrs[g] = shards[g]->d;
    }
    ShardSrc dst = {};
    PoolBlock d_table;
    ZKCHK(shard_src(c, ptrs, dst, d_table));
    ZKCHK(launch_shard_layout(c, true, t->d, dst, lw, t->n_vars));
    for (uint32_t g = 0; g < world; ++g) out[g] = shards[g].release();
    return ZK_OK;
}
extern "C" int32_t zk_mle_interleave(zk_ctx *c, const zk_mle *const *shards, uint32_t world, zk_mle **out) {
    if (!c || !shards || !out) return ZK_ERR_BAD_ARG;
    if (world == 0 || (world & (world - 1)) || world > 65536) return ZK_ERR_BAD_ARG;
    for (uint32_t g = 0; g < world; ++g)
        if (!shards[g]) return ZK_ERR_BAD_ARG;
    std::vector<uint64_t *> ptrs(world);
    for (uint32_t g = 0; g < world; ++g) {
        if (shards[g]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
        if (shards[g]->n_vars != shards[0]->n_vars) return ZK_ERR_ARITY_MISMATCH;
        ptrs[g] = shards[g]->d;
    }
    ZKCHK(use_device(c));
    return shard_interleave(c, ptrs, nullptr, world, shards[0]->n_vars, out);
}
// the shard goes to the device without the rest of the table: host threads (CopyHelpers) gather 16-MiB chunks of it into the
// context's two pinned staging buffers, and the copy of chunk i runs while chunk i + 1 is gathered
extern "C" int32_t zk_mle_upload_shard(zk_ctx *c, uint64_t n_vars, const uint64_t *evals, uint64_t len, uint32_t world, uint32_t rank,
                                       zk_mle **out) {
    if (!c || !out || (!evals && len)) return ZK_ERR_BAD_ARG;
    if (n_vars >= 64 || len != (1ull << n_vars)) return ZK_ERR_EVAL_LEN;   // evaluation_form.rs:19-21
    if (!shard_world_ok(n_vars, world) || rank >= world) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const uint64_t m = 1ull << (n_vars - log2_world(world));
    const uint64_t chunk = m < (1ull << 19) ? m : (1ull << 19);
    const size_t cb = (size_t)chunk * 32;
    MleHolder t;
    ZKCHK(mle_alloc(c, n_vars - log2_world(world), t.put()));
    // an rc chain: the stream is waited for on the failure paths as well (the staging buffers are reused), and the HIP error text
    // is taken once at the end
    int32_t rc = host_staging(c, cb);
    if (rc == ZK_OK) {
        CopyHelpers helpers((size_t)m * 32);
        const uint8_t *src = reinterpret_cast<const uint8_t *>(evals + 4 * (uint64_t)rank);
        for (uint64_t i = 0; i * chunk < m && rc == ZK_OK; ++i) {
            const int b = (int)(i & 1);
            if (i >= 2 && hipEventSynchronize(c->ev_absorb[b]) != hipSuccess) rc = ZK_ERR_HIP;   // its previous copy has left
            if (rc != ZK_OK) break;
            helpers.copy(c->h_absorb[b], src + (size_t)i * cb * world, cb, world);
            if (hipMemcpyAsync(t->d + 4 * i * chunk, c->h_absorb[b], cb, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                hipEventRecord(c->ev_absorb[b], c->stream) != hipSuccess)
                rc = ZK_ERR_HIP;
        }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == ZK_OK) rc = ZK_ERR_HIP;   // the staging buffers are reused
    if (rc != ZK_OK) {
        if (rc == ZK_ERR_HIP) g_hip_err = std::string("upload_shard: ") + hipGetErrorString(hipGetLastError());
        return rc;
    }
    *out = t.release();
    return ZK_OK;
}

static uint64_t bit_reverse64(uint64_t x) {
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    return __builtin_bswap64(x);
}
// the zeta tile kernels use 64 KiB + 128 B of dynamic LDS (two per CU): above the 64-KiB default, so opt in once per device
static int32_t zeta_lds_opt_in(zk_ctx *c) {
    static std::mutex mu;
    static std::set<int> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count(c->device)) return ZK_OK;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_zeta_first), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kZetaLdsBytes));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_zeta_tile), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kZetaLdsBytes));
    done.insert(c->device);
    return ZK_OK;
}
// lists longer than this are ordered on the device (zeta_sort.hip): the host's sort + merge + upload of 2^16 terms took 3.5 ms, six
// times the transform; ZK_ZETA_DEVICE_SORT_MIN overrides (0 = always on the device, tests)
static uint64_t zeta_device_sort_min() {
    static const uint64_t v = env_u64("ZK_ZETA_DEVICE_SORT_MIN", 4096, 0, (uint64_t)1 << 40);
    return v;
}
namespace zk {
int zeta_sort_terms(hipStream_t stream, const uint64_t *d_keys, uint64_t n, uint32_t n_vars, uint64_t *d_idx_unsorted, uint32_t *d_pos_unsorted,
                    uint64_t *d_idx_sorted, uint32_t *d_perm, void *temp, size_t *temp_bytes);
}
// the tiled passes over a table whose first pass has been given its term list
static int32_t zeta_tiled_passes(zk_ctx *c, zk_mle *t, uint64_t n_vars, const uint64_t *d_keys, const uint64_t *d_coeffs, uint64_t m, const uint32_t *d_perm) {
    ZKCHK(zeta_lds_opt_in(c));
    const uint32_t tile_log = n_vars < kZetaTileLog ? (uint32_t)n_vars : kZetaTileLog;
    k_zeta_first<<<(uint32_t)(1ull << (n_vars - tile_log)), kBlock, kZetaLdsBytes, c->stream>>>(t->d, d_keys, d_coeffs, m, tile_log, c->fi->P, d_perm);
    HIPCHK(hipGetLastError());
    const uint32_t rem = (uint32_t)n_vars - tile_log, n_pass = (rem + 7) / 8;
    uint32_t pos = tile_log;
    for (uint32_t p = 0; p < n_pass; ++p) {
        const uint32_t L = rem / n_pass + (p < rem % n_pass ? 1u : 0u);
        k_zeta_tile<<<(uint32_t)(1ull << (n_vars - kZetaTileLog)), kBlock, kZetaLdsBytes, c->stream>>>(t->d, pos, L, c->fi->P);
        HIPCHK(hipGetLastError());
        pos += L;
    }
    return ZK_OK;
}
// long term lists: upload as given, order on the device, sum duplicate keys inside the first pass
static int32_t coeff_to_evaluation_device_sort(zk_ctx *c, uint64_t n_vars, const uint64_t *keys, const uint64_t *coeffs, uint64_t n_terms, zk_mle **out) {
    MleHolder t;
    ZKCHK(mle_alloc(c, n_vars, t.put()));
    // one device block: [keys | idx unsorted | idx sorted | coeffs | pos unsorted | perm | sort scratch]
    size_t temp_bytes = 0;
    if (zeta_sort_terms(c->stream, nullptr, n_terms, (uint32_t)n_vars, nullptr, nullptr, nullptr, nullptr, nullptr, &temp_bytes) != 0) return ZK_ERR_HIP;
    const size_t w8 = (size_t)n_terms * 8, w4 = ((size_t)n_terms * 4 + 7) & ~(size_t)7;
    PoolBlock block;
    ZKCHK(block.alloc(c, 3 * w8 + 4 * w8 + 2 * w4 + ((temp_bytes + 255) & ~(size_t)255) + 256));
    DrainOnExit drain(c);   // on every path: the caller's arrays are read by the copies
    uint8_t *blk = block.as<uint8_t>();
    uint64_t *d_keys = reinterpret_cast<uint64_t *>(blk), *d_idx_u = d_keys + n_terms, *d_idx_s = d_idx_u + n_terms, *d_coeffs = d_idx_s + n_terms;
    uint32_t *d_pos_u = reinterpret_cast<uint32_t *>(blk + 7 * w8), *d_perm = reinterpret_cast<uint32_t *>(blk + 7 * w8 + w4);
    void *temp = blk + 7 * w8 + 2 * w4;
    HIPCHK(hipMemcpyAsync(d_keys, keys, w8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_coeffs, coeffs, 4 * w8, hipMemcpyHostToDevice, c->stream));
    if (zeta_sort_terms(c->stream, d_keys, n_terms, (uint32_t)n_vars, d_idx_u, d_pos_u, d_idx_s, d_perm, temp, &temp_bytes) != 0) return ZK_ERR_HIP;
    ZKCHK(zeta_tiled_passes(c, t.get(), n_vars, d_idx_s, d_coeffs, n_terms, d_perm));
    ZKCHK(drain.wait());
    *out = t.release();
    return ZK_OK;
}
// CoeffMultilinearPolynomial::to_evaluation_form (coefficient_form.rs:340-347): scatter + zeta transform on the device
static int32_t coeff_to_evaluation_impl(zk_ctx *c, uint64_t n_vars, const uint64_t *keys, const uint64_t *coeffs, uint64_t n_terms,
                                        zk_mle **out) {
    if (!c || !out || (n_terms && (!keys || !coeffs))) return ZK_ERR_BAD_ARG;
    if (n_vars == 0 || n_vars > kMaxVars) return ZK_ERR_EVAL_LEN;
    for (uint64_t t = 0; t < n_terms; ++t)
        if (keys[t] >> n_vars) return ZK_ERR_COEFF_RANGE;                            // coefficient_form.rs:183-186
    ZKCHK(use_device(c));
    static const bool global_passes_flag = env_flag("ZK_ZETA_GLOBAL");
    if (!global_passes_flag && n_terms && n_terms >= zeta_device_sort_min() && n_terms < ((uint64_t)1 << 32))
        return coeff_to_evaluation_device_sort(c, n_vars, keys, coeffs, n_terms, out);
    // BTreeMap semantics: one entry per key, duplicate terms summed (coefficient_form.rs:164-171).  Keyed by the TABLE INDEX of the
    // term (key bit v <-> variable v <-> index bit n-1-v: the bit-reversed key), so the list comes out sorted by index, which is
    // what k_zeta_first's per-tile binary search needs.
    std::vector<std::pair<uint64_t, uint64_t>> order(n_terms);   // (table index, position in the caller's list)
    for (uint64_t t = 0; t < n_terms; ++t) order[t] = {bit_reverse64(keys[t]) >> (64 - n_vars), t};
    std::sort(order.begin(), order.end());
    // one staging block: m indices, then m coefficients (4 words each); pinned (the context's results block) while it is small
    const size_t stage_bytes = (size_t)n_terms * 40;
    std::vector<uint64_t> pageable;
    uint64_t *hs = nullptr;
    if (stage_bytes <= ((size_t)1 << 20)) {
        uint8_t *blk = nullptr;
        ZKCHK(results_staging(c, stage_bytes ? stage_bytes : 8, &blk));
        hs = reinterpret_cast<uint64_t *>(blk);
    } else {
        pageable.resize((size_t)n_terms * 5);
        hs = pageable.data();
    }
    uint64_t m = 0;
    {
        uint64_t *hk = hs, *hc = hs + n_terms;   // indices packed at the front; coefficients start at word n_terms (>= m)
        for (uint64_t i = 0; i < n_terms;) {
            Fe acc = fe_from_u64limbs(coeffs + 4 * order[i].second);
            uint64_t j = i + 1;
            for (; j < n_terms && order[j].first == order[i].first; ++j)
                acc = fe_add(acc, fe_from_u64limbs(coeffs + 4 * order[j].second), c->fi->P);
            hk[m] = order[i].first;
            fe_to_u64limbs(acc, hc + 4 * m);
            ++m;
            i = j;
        }
    }
    MleHolder t;
    ZKCHK(mle_alloc(c, n_vars, t.put()));
    PoolBlock terms;
    uint64_t *d_keys = nullptr, *d_coeffs = nullptr;
    if (m) ZKCHK(terms.alloc(c, stage_bytes));
    DrainOnExit drain(c);   // on every path: the host staging vectors go out of scope
    if (m) {
        HIPCHK(hipMemcpyAsync(terms.p, hs, (size_t)(n_terms + 4 * m) * 8, hipMemcpyHostToDevice, c->stream));
        d_keys = terms.as();
        d_coeffs = d_keys + n_terms;
    }
    static const bool global_passes = env_flag("ZK_ZETA_GLOBAL");   // round 4's path (memset + scatter + three bits per launch): A/B only
    if (!global_passes) {
        // LDS-tiled passes (zeta_kernels.cuh): the low min(n, 11) index bits from the term list without reading the table, then
        // the remaining bits in passes of at most 8, evenly split
        ZKCHK(zeta_tiled_passes(c, t.get(), n_vars, d_keys, d_coeffs, m, nullptr));
    } else {
        HIPCHK(hipMemsetAsync(t->d, 0, (size_t)32 << n_vars, c->stream));
        if (m) {
            k_scatter_terms<<<grid_for(m), kBlock, 0, c->stream>>>(d_keys, d_coeffs, m, t->d);
            HIPCHK(hipGetLastError());
        }
        for (uint32_t b = 0; b < n_vars;) {   // the subset-sum butterfly over every index bit, three bits per pass
            const uint32_t v = n_vars - b >= 3 ? 3u : (uint32_t)(n_vars - b);
            const uint64_t groups = 1ull << (n_vars - v);
            uint64_t g = (groups + kBlock - 1) / kBlock;
            if (g > kMaxGridStream) g = kMaxGridStream;
            if (v == 3) k_zeta_multi<3><<<(uint32_t)g, kBlock, 0, c->stream>>>(t->d, groups, b, c->fi->P);
            else if (v == 2) k_zeta_multi<2><<<(uint32_t)g, kBlock, 0, c->stream>>>(t->d, groups, b, c->fi->P);
            else k_zeta_pass<<<(uint32_t)g, kBlock, 0, c->stream>>>(t->d, groups, b, c->fi->P);
            HIPCHK(hipGetLastError());
            b += v;
        }
    }
    ZKCHK(drain.wait());
    *out = t.release();
    return ZK_OK;
}
// the term list is merged in host containers sized by the caller's n_terms: an allocation failure is a status, not an exception
extern "C" int32_t zk_coeff_to_evaluation(zk_ctx *c, uint64_t n_vars, const uint64_t *keys, const uint64_t *coeffs, uint64_t n_terms,
                                          zk_mle **out) {
    try {
        return coeff_to_evaluation_impl(c, n_vars, keys, coeffs, n_terms, out);
    } catch (const std::bad_alloc &) {
        return ZK_ERR_ALLOC;
    } catch (...) {
        return ZK_ERR_BAD_ARG;
    }
}

// ------------------------------------------------------------------------------------------------------------
// ProductPoly
// ------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_product_check(const zk_mle *const *f, uint64_t k) {
    if (k == 0) return ZK_ERR_EMPTY_PRODUCT;   // product_poly.rs:15-17
    if (!f) return ZK_ERR_BAD_ARG;
    for (uint64_t i = 0; i < k; ++i) {
        if (!f[i]) return ZK_ERR_BAD_ARG;
        if (f[i]->n_vars != f[0]->n_vars) return ZK_ERR_ARITY_MISMATCH;   // product_poly.rs:20-26
        if (f[i]->ctx != f[0]->ctx) return ZK_ERR_CONTEXT_MISMATCH;
    }
    return ZK_OK;
}
int32_t zk::product_args(zk_ctx *c, const zk_mle *const *f, uint64_t k) {
    if (!c) return ZK_ERR_BAD_ARG;
    ZKCHK(zk_product_check(f, k));
    if (f[0]->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (k > (uint64_t)kMaxFactors) return ZK_ERR_UNSUPPORTED;
    return use_device(c);
}

extern "C" int32_t zk_prod_reduce(zk_ctx *c, const zk_mle *const *f, uint64_t k, zk_mle **out) {
    if (!out) return ZK_ERR_BAD_ARG;
    ZKCHK(product_args(c, f, k));
    zk_mle *o = nullptr;
    ZKCHK(mle_alloc(c, f[0]->n_vars, &o));
    FactorPtrs fp = {};
    for (uint64_t i = 0; i < k; ++i) fp.in[i] = f[i]->d;
    const uint64_t n = 1ull << f[0]->n_vars;
    if (n >= 64) {
        uint64_t g = n / kBlock;   // one 64-element run per wave and pass
        if (g > 2 * kMaxGridStream) g = 2 * kMaxGridStream;
        k_prod_reduce_run<<<(uint32_t)(g ? g : 1), kBlock, 0, c->stream>>>(fp, (int)k, n, o->d, c->fi->P);
    } else {
        k_prod_reduce<<<grid_for(n), kBlock, 0, c->stream>>>(fp, (int)k, n, o->d, c->fi->P);
    }
    HIPCHK(hipGetLastError());
    *out = o;
    return ZK_OK;
}

extern "C" int32_t zk_product_evaluate(zk_ctx *c, const zk_mle *const *f, uint64_t k, const uint64_t *point,
                                       uint64_t n_point, uint64_t out[4]) {
    if (!out || (!point && n_point)) return ZK_ERR_BAD_ARG;
    ZKCHK(product_args(c, f, k));
    if (n_point != f[0]->n_vars) return ZK_ERR_EVAL_ARITY;   // product_poly.rs:37-39
    Fe prod = fe_one(c->fi->P);
    for (uint64_t i = 0; i < k; ++i) {                       // product_poly.rs:41-43
        uint64_t v[4];
        ZKCHK(zk_mle_evaluate(c, f[i], point, n_point, v));
        prod = fe_mul(prod, fe_from_u64limbs(v), c->fi->P);
    }
    fe_to_u64limbs(prod, out);
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Transcript (host)
// ------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_transcript_new(zk_transcript **out) {
    if (!out) return ZK_ERR_BAD_ARG;
    zk_transcript *t = new (std::nothrow) zk_transcript();
    if (!t) return ZK_ERR_ALLOC;
    t->sp.init();
    *out = t;
    return ZK_OK;
}
extern "C" int32_t zk_transcript_free(zk_transcript *t) {
    delete t;
    return ZK_OK;
}
extern "C" int32_t zk_transcript_append(zk_transcript *t, const uint8_t *data, size_t len) {
    if (!t || (!data && len)) return ZK_ERR_BAD_ARG;
    t->sp.update(data, len);
    return ZK_OK;
}
extern "C" int32_t zk_transcript_sample_challenge(zk_transcript *t, uint8_t out[32]) {
    if (!t || !out) return ZK_ERR_BAD_ARG;
    t->sp.sample_challenge(out);
    return ZK_OK;
}
extern "C" int32_t zk_transcript_sample_field_element(zk_transcript *t, int32_t field, uint64_t out[4]) {
    if (!t || !out) return ZK_ERR_BAD_ARG;
    const FieldInfo *fi = field_info(field);
    if (!fi) return ZK_ERR_BAD_FIELD;
    uint8_t h[32];
    t->sp.sample_challenge(h);                                           // transcript/src/lib.rs:28
    fe_to_u64limbs(fe_from_be_bytes_mod_order(h, 32, fi->P), out);       // :29
    return ZK_OK;
}
extern "C" int32_t zk_transcript_sample_n_field_elements(zk_transcript *t, int32_t field, uint64_t n, uint64_t *out) {
    if (!t || (!out && n)) return ZK_ERR_BAD_ARG;
    if (!field_info(field)) return ZK_ERR_BAD_FIELD;
    for (uint64_t i = 0; i < n; ++i) ZKCHK(zk_transcript_sample_field_element(t, field, out + 4 * i));   // transcript/src/lib.rs:32-34
    return ZK_OK;
}
extern "C" int32_t zk_keccak256(const uint8_t *data, size_t len, uint8_t out[32]) {
    if ((!data && len) || !out) return ZK_ERR_BAD_ARG;
    Sponge s;
    s.init();
    s.update(data, len);
    s.finalize_reset(out);
    return ZK_OK;
}

void zk::absorb_elements(Sponge &sp, const uint64_t *elems, uint64_t n, const FieldParams &P) {   // sumcheck/src/lib.rs:23-29
    uint8_t b[32];
    for (uint64_t i = 0; i < n; ++i) {
        fe_to_bytes_be(fe_from_u64limbs(elems + 4 * i), P, b);
        sp.update(b, 32);
    }
}
Fe zk::squeeze_field_element(Sponge &sp, const FieldParams &P) {   // transcript/src/lib.rs:27-30
    uint8_t h[32];
    sp.sample_challenge(h);
    return fe_from_be_bytes_mod_order(h, 32, P);
}
// pinned staging for results, grown on demand
int32_t zk::results_staging(zk_ctx *c, size_t bytes, uint8_t **out) {
    if (c->h_results_bytes < bytes) {
        if (c->h_results) (void)hipHostFree(c->h_results);
        c->h_results = nullptr;
        c->h_results_bytes = 0;
        size_t cap = 1 << 16;
        while (cap < bytes) cap <<= 1;
        HIPCHK(hipHostMalloc((void **)&c->h_results, cap, kPolledHostFlags));
        c->h_results_bytes = cap;
    }
    *out = c->h_results;
    return ZK_OK;
}
// the context's two pinned staging buffers (at least cb bytes each, kept across calls) and their events
int32_t zk::host_staging(zk_ctx *c, size_t cb) {
    if (c->h_absorb_bytes < cb) {
        for (int b = 0; b < 2; ++b) {
            if (c->h_absorb[b]) (void)hipHostFree(c->h_absorb[b]);
            c->h_absorb[b] = nullptr;
        }
        c->h_absorb_bytes = 0;
        for (int b = 0; b < 2; ++b) HIPCHK(hipHostMalloc((void **)&c->h_absorb[b], cb, hipHostMallocDefault));
        c->h_absorb_bytes = cb;
    }
    if (!c->ev_absorb[0])
        for (int b = 0; b < 2; ++b) HIPCHK(hipEventCreateWithFlags(&c->ev_absorb[b], hipEventDisableTiming));
    return ZK_OK;
}
// absorb poly.to_bytes() (product_poly.rs:77-83) -- device serialiser, chunked D2H, host sponge.  The Keccak sponge is
// serial by construction and runs on the host (one GPU wave permutes 136 bytes in ~3 us = 45 MB/s; a host core does
// 0.4-0.75 GB/s with keccak_host::rounds), so it bounds `prove`; the serialiser kernel and the copy of chunk i+1 run while the host absorbs
// chunk i (two device + two pinned buffers, one event each; the pinned buffers stay with the context).
// consume(host_ptr, bytes) is called once per 16-MiB chunk, in order, on the calling thread, while the next chunk is serialised and copied
int32_t zk::stream_table_bytes(zk_ctx *c, const zk_mle *const *f, uint64_t k, const std::function<void(const uint8_t *, size_t)> &consume) {
    const uint64_t n = 1ull << f[0]->n_vars;
    const uint64_t chunk = n < (1ull << 19) ? n : (1ull << 19);   // 16 MiB of bytes per chunk
    const size_t cb = (size_t)chunk * 32;
    const uint64_t per_table = n / chunk, total = per_table * k;
    ZKCHK(host_staging(c, cb));
    PoolBlock d_bytes[2];
    ZKCHK(d_bytes[0].alloc(c, cb));
    ZKCHK(d_bytes[1].alloc(c, cb));
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the double buffers go back to the pool
    auto enqueue = [&](uint64_t i) -> int32_t {
        const int b = (int)(i & 1);
        const uint64_t *src = f[i / per_table]->d + 4 * (i % per_table) * chunk;
        k_to_bytes<<<grid_for(chunk), kBlock, 0, c->stream>>>(src, d_bytes[b].as<uint8_t>(), chunk, c->fi->P);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c->h_absorb[b], d_bytes[b].p, cb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(c->ev_absorb[b], c->stream));
        return ZK_OK;
    };
    ZKCHK(enqueue(0));
    for (uint64_t i = 0; i < total; ++i) {
        if (i + 1 < total) ZKCHK(enqueue(i + 1));   // its buffers were released when chunk i-1 was consumed
        HIPCHK(hipEventSynchronize(c->ev_absorb[i & 1]));
        consume(c->h_absorb[i & 1], cb);
    }
    drain.armed = false;   // every chunk has been consumed: nothing of this call is left on the stream
    return ZK_OK;
}

// plain device <-> host copies on the context's stream (synchronous): lets a host without a HIP binding (tests, the
// single-process rehearsal of the sharded prover) move the lanes / tail buffers
extern "C" int32_t zk_ctx_memcpy_dtoh(zk_ctx *c, void *dst_host, const void *src_dev, uint64_t bytes) {
    if (!c || !dst_host || !src_dev) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    HIPCHK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
extern "C" int32_t zk_ctx_memcpy_htod(zk_ctx *c, void *dst_dev, const void *src_host, uint64_t bytes) {
    if (!c || !dst_dev || !src_host) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
extern "C" int32_t zk_ctx_device_alloc(zk_ctx *c, uint64_t bytes, void **out) {
    if (!c || !out) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    PoolBlock blk;
    ZKCHK(blk.alloc(c, bytes));
    *out = blk.release();   // the caller owns it and names its size again in zk_ctx_device_free
    return ZK_OK;
}
extern "C" int32_t zk_ctx_device_free(zk_ctx *c, void *ptr, uint64_t bytes) {
    if (!c) return ZK_ERR_BAD_ARG;
    pool_free(c, ptr, bytes);
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// measurement hooks
// ------------------------------------------------------------------------------------------------------------
extern "C" int32_t zk_bench_fold(zk_ctx *c, const zk_mle *t, const uint64_t r[4], zk_mle *out, int32_t reps, double *out_ms) {
    if (!c || !t || !r || !out || !out_ms || reps <= 0) return ZK_ERR_BAD_ARG;
    if (t->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (t->n_vars == 0 || out->n_vars != t->n_vars - 1) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const Fe rr = fe_from_u64limbs(r);
    return timed_span(c, 0, AfterWarm::kNoWait, reps, [&] { return launch_fold(c, t->d, out->d, t->n_vars, 0, rr); }, out_ms);
}
// the same with one event per launch boundary: out_ms_each[i] = duration of launch i (reps values); median / min / mean are
// the caller's to take (report median and min)
extern "C" int32_t zk_bench_fold_samples(zk_ctx *c, const zk_mle *t, const uint64_t r[4], zk_mle *out, int32_t reps, int32_t group,
                                         double *out_ms_each) {
    if (!c || !t || !r || !out || !out_ms_each || reps <= 0 || group <= 0 || reps > (1 << 20)) return ZK_ERR_BAD_ARG;
    if (t->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (t->n_vars == 0 || out->n_vars != t->n_vars - 1) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    const Fe rr = fe_from_u64limbs(r);
    // an event record costs the stream ~4 us (r02: 22.5 vs 17.3 us per step on a 2^21 shard), so a sample may span `group` launches
    const int n_samples = (reps + group - 1) / group;
    if (n_samples > 65536) return ZK_ERR_BAD_ARG;
    PhaseEvents ev(c);   // n_samples + 1 events: sample i lies between event i and event i + 1
    ZKCHK(ev.create((size_t)n_samples - 1));
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the events go
    ZKCHK(ev.begin());
    for (int i = 0; i < reps; ++i) {
        ZKCHK(launch_fold(c, t->d, out->d, t->n_vars, 0, rr));
        if (i + 1 == reps) ZKCHK(ev.end());   // the last group may be short
        else if ((i + 1) % group == 0) ZKCHK(ev.mark((size_t)(i / group)));
    }
    drain.armed = false;   // the last event has been waited for
    for (int i = 0; i < n_samples; ++i) {
        double ms = 0.0;
        ZKCHK(ev.span_ms((size_t)i, (size_t)i + 1, &ms));
        const int launches = i + 1 < n_samples ? group : reps - i * group;
        out_ms_each[i] = ms / launches;
    }
    return ZK_OK;
}
extern "C" int32_t zk_bench_evaluate(zk_ctx *c, const zk_mle *t, const uint64_t *point, uint64_t n_point, int32_t reps, double *out_ms_each) {
    if (!c || !t || !out_ms_each || reps <= 0) return ZK_ERR_BAD_ARG;
    uint64_t out[4];
    return wall_clock_each(c, reps, [&] { return zk_mle_evaluate(c, t, point, n_point, out); }, out_ms_each);
}
// device time of evaluate: `reps` back-to-back enqueues of its launches (no host wait in between) between two HIP events on the
// context's stream -> average ms per evaluate.  What the roofline of the streaming kernel is priced on (bench.py roofline_evaluate).
extern "C" int32_t zk_bench_evaluate_device(zk_ctx *c, const zk_mle *t, const uint64_t *point, uint64_t n_point, int32_t reps, double *out_ms) {
    if (!c || !t || !out_ms || reps <= 0 || (!point && n_point)) return ZK_ERR_BAD_ARG;
    if (t->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (n_point != t->n_vars) return ZK_ERR_EVAL_ARITY;
    ZKCHK(use_device(c));
    // one warm call: scratch from the pool
    return timed_span(c, 1, AfterWarm::kWait, reps, [&] { return evaluate_device(c, t, point, c->d_sums); }, out_ms);
}
extern "C" int32_t zk_bench_modmul(zk_ctx *c, int32_t variant, int32_t iters, double *out) {
    if (!c || !out || iters <= 0) return ZK_ERR_BAD_ARG;
    if (variant != 0 && variant != 1) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    const uint32_t blocks = 256 * 8;
    Fe seed = c->fi->two_adic_root;
    const Mul29 seed29 = mul29_prepare(seed, c->fi->P);
    k_bench_modmul<<<blocks, kBlock, 0, c->stream>>>(c->d_sums, 8, c->fi->P, seed, seed29, variant);   // warm-up
    double ms = 0.0;
    ZKCHK(timed_span(c, 0, AfterWarm::kNoWait, 1, [&] {
        k_bench_modmul<<<blocks, kBlock, 0, c->stream>>>(c->d_sums, iters, c->fi->P, seed, seed29, variant);
        return ZK_OK;
    }, &ms));
    *out = (double)blocks * kBlock * 2.0 * iters / (ms * 1e-3);
    return ZK_OK;
}
extern "C" int32_t zk_bench_copy(zk_ctx *c, uint64_t bytes, int32_t reps, double *out_gbps) {
    if (!c || !out_gbps || reps <= 0 || bytes < 16) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    RawBlock a_block, b_block;
    if (hipMalloc(a_block.put(), bytes) != hipSuccess || hipMalloc(b_block.put(), bytes) != hipSuccess) return ZK_ERR_ALLOC;
    uint4 *a = static_cast<uint4 *>(a_block.get()), *b = static_cast<uint4 *>(b_block.get());
    HIPCHK(hipMemsetAsync(a, 1, bytes, c->stream));
    const uint64_t n16 = bytes / 16;
    k_bench_copy<<<kMaxGrid, kBlock, 0, c->stream>>>(a, b, n16);   // warm-up
    double ms = 0.0;   // per launch
    ZKCHK(timed_span(c, 0, AfterWarm::kNoWait, reps, [&] {
        k_bench_copy<<<kMaxGrid, kBlock, 0, c->stream>>>(a, b, n16);
        return ZK_OK;
    }, &ms));   // (a failed span has drained the stream before the two blocks are freed)
    *out_gbps = 2.0 * (double)n16 * 16.0 / (ms * 1e-3) / 1e9;
    return ZK_OK;
}

