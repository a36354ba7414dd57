// cmle.hip -- host side of the dense CoeffMultilinearPolynomial (coefficient_form.rs; kernels in cmle_kernels.cuh).  It shares the
// context's pool, the MLE evaluator and the to_bytes staging with the rest of the library (host_core.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "copy_helpers.hpp"
#include "env.hpp"
#include "cmle_kernels.cuh"

// The coefficients of CoeffMultilinearPolynomial (coefficient_form.rs:27-30, selector_to_index :418-430) at the present keys
// {k < 2^n_vars : k & fixed == 0}, ascending: 2^log_len of them, log_len = n_vars - popcount(fixed); entry j is key pdep(j, ~fixed).
// fixed == 0 (what upload and interpolate make): every key, index = key.  partial_evaluate sets bits of `fixed`, relabel clears them.
struct zk_cmle {
    zk_ctx *ctx;
    uint64_t n_vars;
    uint64_t *d;   // a pool block of 32 << log_len bytes (the tables' size classes)
    uint64_t fixed;
    uint64_t log_len;
};

static int32_t cmle_alloc(zk_ctx *c, uint64_t n_vars, zk_cmle **out, uint64_t fixed = 0) {
    if (n_vars > kMaxVars) return ZK_ERR_UNSUPPORTED;
    zk_cmle *p = new (std::nothrow) zk_cmle();
    if (!p) return ZK_ERR_ALLOC;
    p->ctx = c;
    p->n_vars = n_vars;
    p->fixed = fixed;
    p->log_len = n_vars - (uint64_t)__builtin_popcountll(fixed);
    PoolBlock blk;
    const int32_t rc = blk.alloc(c, mle_block_bytes(p->log_len));
    if (rc != ZK_OK) {
        delete p;
        return rc;
    }
    p->d = static_cast<uint64_t *>(blk.release());   // the handle owns the block from here on (cmle_release)
    *out = p;
    return ZK_OK;
}
static void cmle_release(zk_cmle *p) {
    if (!p) return;
    pool_free(p->ctx, p->d, mle_block_bytes(p->log_len));
    delete p;
}
using CmleHolder = Scoped<zk_cmle, cmle_release>;
// the tile kernels use the zeta passes' 64 KiB + 128 B of dynamic LDS: opt in once per device
static int32_t cmle_lds_opt_in(zk_ctx *c) {
    static std::mutex mu;
    static std::set<int> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count(c->device)) return ZK_OK;
    const void *fns[4] = {reinterpret_cast<const void *>(&k_cmle_first<true>), reinterpret_cast<const void *>(&k_cmle_first<false>),
                          reinterpret_cast<const void *>(&k_cmle_tile<true>), reinterpret_cast<const void *>(&k_cmle_tile<false>)};
    for (const void *f : fns) HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kZetaLdsBytes));
    done.insert(c->device);
    return ZK_OK;
}
// out[brev_n(j)] = (Moebius if sub, else zeta)(in)[j] over 2^n entries; in entries at index >= in_len count as zero.  Out of place.
// Pass 1 does the low lo and high hi index bits, the rest go in passes of at most 8 bits, evenly split (cmle_kernels.cuh).
static int32_t cmle_transform(zk_ctx *c, const uint64_t *in, uint64_t in_len, uint64_t *out, uint32_t n, bool sub) {
    ZKCHK(cmle_lds_opt_in(c));
    const uint32_t lo = n >= kZetaTileLog ? kCmleFirstLo : n / 2, hi = n >= kZetaTileLog ? kCmleFirstHi : n - n / 2;
    const uint32_t grid1 = 1u << (n - lo - hi);
    if (sub) k_cmle_first<true><<<grid1, kBlock, kZetaLdsBytes, c->stream>>>(in, out, in_len, n, lo, hi, c->fi->P);
    else k_cmle_first<false><<<grid1, kBlock, kZetaLdsBytes, c->stream>>>(in, out, in_len, n, lo, hi, c->fi->P);
    HIPCHK(hipGetLastError());
    const uint32_t rem = n - lo - hi, n_pass = (rem + 7) / 8;
    uint32_t pos = hi;
    for (uint32_t p = 0; p < n_pass; ++p) {
        const uint32_t L = rem / n_pass + (p < rem % n_pass ? 1u : 0u);
        const uint32_t log_c = pos < kZetaTileLog - L ? pos : kZetaTileLog - L;
        const uint32_t grid = 1u << (n - L - log_c);
        if (sub) k_cmle_tile<true><<<grid, kBlock, kZetaLdsBytes, c->stream>>>(out, pos, L, log_c, c->fi->P);
        else k_cmle_tile<false><<<grid, kBlock, kZetaLdsBytes, c->stream>>>(out, pos, L, log_c, c->fi->P);
        HIPCHK(hipGetLastError());
        pos += L;
    }
    return ZK_OK;
}
// bit_count_for_n_elem (coefficient_form.rs:517-523): the length of format!("{:b}", len - 1), so 1 for len 1 (len >= 1)
static uint64_t cmle_n_vars_for_len(uint64_t len) {
    const uint64_t x = len - 1;
    return x ? 64 - (uint64_t)__builtin_clzll(x) : 1;
}

extern "C" int32_t zk_cmle_upload(zk_ctx *c, uint64_t n_vars, const uint64_t *coeffs, uint64_t len, zk_cmle **out) {
    if (!c || !out || (!coeffs && len)) return ZK_ERR_BAD_ARG;
    if (n_vars >= 64 || len != (1ull << n_vars)) return ZK_ERR_EVAL_LEN;
    if (n_vars > kMaxVars) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    CmleHolder p;
    ZKCHK(cmle_alloc(c, n_vars, p.put()));
    hipError_t e = hipMemcpyAsync(p->d, coeffs, (size_t)len * 32, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        g_hip_err = std::string("cmle upload: ") + hipGetErrorString(e);
        return ZK_ERR_HIP;
    }
    *out = p.release();
    return ZK_OK;
}
extern "C" int32_t zk_cmle_download(zk_ctx *c, const zk_cmle *p, uint64_t *out) {
    if (!c || !p || !out) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    HIPCHK(hipMemcpyAsync(out, p->d, (size_t)32 << p->log_len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
extern "C" int32_t zk_cmle_n_vars(const zk_cmle *p, uint64_t *out) {
    if (!p || !out) return ZK_ERR_BAD_ARG;
    *out = p->n_vars;
    return ZK_OK;
}
extern "C" int32_t zk_cmle_free(zk_ctx *c, zk_cmle *p) {
    if (!p) return ZK_OK;
    if (!c) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    cmle_release(p);   // back to the context's pool; reuse is stream-ordered
    return ZK_OK;
}

// CoeffMultilinearPolynomial::interpolate (coefficient_form.rs:200-216) of a resident table
extern "C" int32_t zk_cmle_interpolate(zk_ctx *c, const zk_mle *values, zk_cmle **out) {
    if (!c || !values || !out) return ZK_ERR_BAD_ARG;
    if (values->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const uint64_t n = values->n_vars ? values->n_vars : 1;   // one value: n_vars 1, the second value counts as zero
    ZKCHK(use_device(c));
    CmleHolder p;
    ZKCHK(cmle_alloc(c, n, p.put()));
    ZKCHK(cmle_transform(c, values->d, 1ull << values->n_vars, p->d, (uint32_t)n, true));
    *out = p.release();
    return ZK_OK;
}
int32_t zk::cmle_interpolate_into(zk_ctx *c, const zk_mle *values, uint64_t *d_coeffs) {
    return cmle_transform(c, values->d, 1ull << values->n_vars, d_coeffs, (uint32_t)values->n_vars, true);
}
extern "C" int32_t zk_cmle_interpolate_host(zk_ctx *c, const uint64_t *values, uint64_t len, uint64_t *out_n_vars, uint64_t *out_coeffs) {
    if (!c || !out_n_vars || (len && (!values || !out_coeffs))) return ZK_ERR_BAD_ARG;
    if (len > (1ull << kMaxVars)) return ZK_ERR_UNSUPPORTED;
    if (len == 0) {   // Self::new(0, vec![]): no variable, no key
        *out_n_vars = 0;
        return ZK_OK;
    }
    const uint64_t n = cmle_n_vars_for_len(len);
    ZKCHK(use_device(c));
    PoolBlock d_in;
    ZKCHK(d_in.alloc(c, (size_t)len * 32));
    CmleHolder p;
    DrainOnExit drain(c);   // on every path: the copies read and write the caller's arrays, and the blocks go back after them
    ZKCHK(cmle_alloc(c, n, p.put()));
    HIPCHK(hipMemcpyAsync(d_in.p, values, (size_t)len * 32, hipMemcpyHostToDevice, c->stream));
    ZKCHK(cmle_transform(c, d_in.as(), len, p->d, (uint32_t)n, true));
    HIPCHK(hipMemcpyAsync(out_coeffs, p->d, (size_t)32 << n, hipMemcpyDeviceToHost, c->stream));
    ZKCHK(drain.wait());
    *out_n_vars = n;
    return ZK_OK;
}
// CoeffMultilinearPolynomial::to_evaluation_form (coefficient_form.rs:340-347) of the dense vector
extern "C" int32_t zk_cmle_to_evaluation(zk_ctx *c, const zk_cmle *p, zk_mle **out) {
    if (!c || !p || !out) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (p->fixed) return ZK_ERR_UNSUPPORTED;      // keys are missing: relabel first (the table of the variables that are left)
    if (p->n_vars == 0) return ZK_ERR_EVAL_LEN;   // as zk_coeff_to_evaluation: an empty vector is no table
    ZKCHK(use_device(c));
    MleHolder t;
    ZKCHK(mle_alloc(c, p->n_vars, t.put()));
    ZKCHK(cmle_transform(c, p->d, 1ull << p->n_vars, t->d, (uint32_t)p->n_vars, false));
    *out = t.release();
    return ZK_OK;
}

// evaluate_slice (coefficient_form.rs:39-69), n_vars >= 1 and n_point >= n_vars: sum_k c_k prod_{v in k} r_v.  The variables with
// r_v = -1 are folded out first (c[k] - c[k | 2^v], highest first so the lower keys keep their bits); the others have weights
// (1, r) = (1 + r)(1 - r', r'), r' = r / (1 + r) (one batched inversion), so what is left is the MLE evaluation of the folded vector
// read as a table -- its index bit n'-1-w <-> point'[w], hence the reversed point -- times prod (1 + r_v).  Enqueues the folds;
// fills `view` (the vector evaluate_device is to read), `pt` and `scale`; `blocks` own the folded vectors and give them back (stream-ordered
// reuse) when the plan dies, after the evaluation is enqueued.
struct CmleEvalPlan {
    zk_mle view;
    std::vector<uint64_t> pt;
    Fe scale;
    std::vector<PoolBlock> blocks;   // (one per variable at -1: more than a PoolScope holds; the plan allocates on the host anyway)
};
static int32_t cmle_evaluate_prepare(zk_ctx *c, const uint64_t *d, uint64_t n, const uint64_t *point, CmleEvalPlan &plan) {
    const FieldParams &P = c->fi->P;
    const Fe one = fe_one(P);
    std::vector<uint32_t> kept, minus;
    std::vector<Fe> r, s;   // kept variables: r_v and 1 + r_v
    for (uint64_t v = 0; v < n; ++v) {
        const Fe rv = fe_from_u64limbs(point + 4 * v), sv = fe_add(one, rv, P);
        if (fe_is_zero(sv)) {
            minus.push_back((uint32_t)v);
        } else {
            kept.push_back((uint32_t)v);
            r.push_back(rv);
            s.push_back(sv);
        }
    }
    // batched inversion of the s: prefix products, one inversion, back
    const size_t nk = kept.size();
    std::vector<Fe> pre(nk);
    Fe acc = one;
    for (size_t i = 0; i < nk; ++i) pre[i] = acc = fe_mul(acc, s[i], P);
    plan.scale = acc;
    Fe inv = nk ? fe_inverse(acc, P) : one;
    plan.pt.assign(4 * nk, 0);
    for (size_t i = nk; i-- > 0;) {
        const Fe s_inv = i ? fe_mul(inv, pre[i - 1], P) : inv;
        inv = fe_mul(inv, s[i], P);
        fe_to_u64limbs(fe_mul(r[i], s_inv, P), &plan.pt[4 * (nk - 1 - i)]);   // point'[w] <-> kept variable nk-1-w
    }
    const uint64_t *src = d;
    uint64_t cur = n;
    for (size_t i = minus.size(); i-- > 0;) {
        const uint64_t n_out = 1ull << (cur - 1);
        plan.blocks.emplace_back();
        ZKCHK(plan.blocks.back().alloc(c, (size_t)n_out * 32));
        uint64_t *dst = plan.blocks.back().as();
        k_cmle_fold_minus_one<<<grid_for(n_out), kBlock, 0, c->stream>>>(src, dst, n_out, minus[i], P);
        HIPCHK(hipGetLastError());
        src = dst;
        --cur;
    }
    plan.view.ctx = c;
    plan.view.n_vars = cur;
    plan.view.d = const_cast<uint64_t *>(src);
    return ZK_OK;
}
static int32_t cmle_evaluate_impl(zk_ctx *c, const zk_cmle *p, const uint64_t *point, uint64_t n_point, uint64_t out[4]) {
    if (!c || !p || !out || (!point && n_point)) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (p->n_vars == 0) return zk_cmle_download(c, p, out);   // the coefficient of key 0 (:44-46)
    if (n_point < p->n_vars) return ZK_ERR_EVAL_ASSIGNMENT;   // :48-50; assignments past n_vars are ignored (:53)
    if (p->log_len == 0) return zk_cmle_download(c, p, out);   // every variable fixed: the constant that is left
    ZKCHK(use_device(c));
    std::vector<uint64_t> left;   // on a partially evaluated handle the fixed variables' coordinates are ignored: no key has their bit
    if (p->fixed) {
        for (uint64_t v = 0; v < p->n_vars; ++v)
            if (!(p->fixed >> v & 1)) left.insert(left.end(), point + 4 * v, point + 4 * v + 4);
        point = left.data();
    }
    CmleEvalPlan plan;
    DrainOnExit drain(c);   // a failed call waits for the folds it enqueued before the plan's blocks go back
    ZKCHK(cmle_evaluate_prepare(c, p->d, p->log_len, point, plan));
    uint64_t res[4] = {0, 0, 0, 0};
    ZKCHK(zk_mle_evaluate(c, &plan.view, plan.pt.data(), plan.view.n_vars, res));   // one host wait
    drain.armed = false;   // the evaluation has waited for everything
    fe_to_u64limbs(fe_mul(fe_from_u64limbs(res), plan.scale, c->fi->P), out);
    return ZK_OK;
}
extern "C" int32_t zk_cmle_evaluate(zk_ctx *c, const zk_cmle *p, const uint64_t *point, uint64_t n_point, uint64_t out[4]) {
    try {   // host vectors sized by n_vars: an allocation failure is a status, not an exception
        return cmle_evaluate_impl(c, p, point, n_point, out);
    } catch (const std::bad_alloc &) {
        return ZK_ERR_ALLOC;
    }
}

// to_bytes (coefficient_form.rs:131-139): the n_vars word, then 40-byte records made on the device in chunks of 2^19 keys, each copied
// to pinned staging while the host copies the previous one out (the two buffers and events of stream_table_bytes)
extern "C" int32_t zk_cmle_to_bytes(zk_ctx *c, const zk_cmle *p, uint8_t *out) {
    if (!c || !p || !out) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    const uint32_t nv = (uint32_t)p->n_vars;
    out[0] = (uint8_t)(nv >> 24), out[1] = (uint8_t)(nv >> 16), out[2] = (uint8_t)(nv >> 8), out[3] = (uint8_t)nv;
    const uint64_t present = p->fixed ? ~p->fixed & ((1ull << nv) - 1) : 0;   // (0 on a handle with every key: index = key)
    const uint64_t n = 1ull << p->log_len, chunk = n < (1ull << 19) ? n : (1ull << 19), total = n / chunk;
    const size_t cb = (size_t)chunk * 40;
    ZKCHK(host_staging(c, cb));
    PoolBlock d_bytes[2];
    ZKCHK(d_bytes[0].alloc(c, cb));
    ZKCHK(d_bytes[1].alloc(c, cb));
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the double buffers go back to the pool
    auto enqueue = [&](uint64_t i) -> int32_t {
        const int b = (int)(i & 1);
        k_cmle_records<<<grid_for(chunk), kBlock, 0, c->stream>>>(p->d + 4 * i * chunk, d_bytes[b].as<uint8_t>(), i * chunk, chunk, c->fi->P, present);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c->h_absorb[b], d_bytes[b].p, cb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(c->ev_absorb[b], c->stream));
        return ZK_OK;
    };
    CopyHelpers helpers((size_t)n * 40);   // (joined before the wait of a failed call: declared after drain)
    ZKCHK(enqueue(0));
    for (uint64_t i = 0; i < total; ++i) {
        if (i + 1 < total) ZKCHK(enqueue(i + 1));   // its buffers were released when chunk i-1 was copied out
        HIPCHK(hipEventSynchronize(c->ev_absorb[i & 1]));
        helpers.copy(out + 4 + (size_t)i * cb, c->h_absorb[i & 1], cb);
    }
    drain.armed = false;   // every chunk has been copied out: nothing of this call is left on the stream
    return ZK_OK;
}

// device time of interpolate (op 0, of t), to_evaluation (op 1, of p) and evaluate (op 2, of p at point): `reps` enqueues between two
// HIP events; the output blocks come from the pool once and are reused by every rep
extern "C" int32_t zk_bench_cmle(zk_ctx *c, int32_t op, const zk_mle *t, const zk_cmle *p, const uint64_t *point, uint64_t n_point, int32_t reps,
                                 double *out_ms) {
    if (!c || !out_ms || reps < 1 || op < 0 || op > 2) return ZK_ERR_BAD_ARG;
    if ((op == 0 && !t) || (op != 0 && !p) || (op == 2 && !point && n_point)) return ZK_ERR_BAD_ARG;
    if ((t && t->ctx != c) || (p && p->ctx != c)) return ZK_ERR_CONTEXT_MISMATCH;
    if (p && p->fixed) return ZK_ERR_UNSUPPORTED;   // times the calls on a handle with every key
    if (op == 1 && p->n_vars == 0) return ZK_ERR_EVAL_LEN;
    if (op == 2 && (p->n_vars == 0 || n_point < p->n_vars)) return ZK_ERR_EVAL_ASSIGNMENT;
    ZKCHK(use_device(c));
    const uint64_t n = op == 0 ? (t->n_vars ? t->n_vars : 1) : p->n_vars;
    PoolBlock o_block;
    if (op != 2) ZKCHK(o_block.alloc(c, (size_t)32 << n));
    uint64_t *const o = o_block.as();
    auto once = [&]() -> int32_t {
        if (op == 0) return cmle_transform(c, t->d, 1ull << t->n_vars, o, (uint32_t)n, true);
        if (op == 1) return cmle_transform(c, p->d, 1ull << n, o, (uint32_t)n, false);
        CmleEvalPlan plan;   // its blocks go back once the evaluation is enqueued: stream-ordered reuse
        ZKCHK(cmle_evaluate_prepare(c, p->d, p->n_vars, point, plan));
        return evaluate_device(c, &plan.view, plan.pt.data(), c->d_sums);
    };
    return timed_span(c, 1, AfterWarm::kWait, reps, once, out_ms);   // one warm call: pool blocks, LDS opt-in
}

// ---- algebra: partial_evaluate, relabel, scalar_multiply, Add, Mul (kernels and the compact index in cmle_kernels.cuh) ----------------
extern "C" int32_t zk_cmle_fixed_mask(const zk_cmle *p, uint64_t *out) {
    if (!p || !out) return ZK_ERR_BAD_ARG;
    *out = p->fixed;
    return ZK_OK;
}
extern "C" int32_t zk_cmle_len(const zk_cmle *p, uint64_t *out) {
    if (!p || !out) return ZK_ERR_BAD_ARG;
    *out = 1ull << p->log_len;
    return ZK_OK;
}
static inline uint32_t cmle_stream_grid(uint64_t items) {
    const uint64_t b = (items + kBlock - 1) / kBlock;
    return (uint32_t)(b < 1 ? 1 : b > kMaxGridStream ? kMaxGridStream : b);
}
// Contracts the compact positions pos[0] > pos[1] > ... (s of them, values val[i]) out of the 2^m entries at src into dst (2^(m - s)
// entries), three per pass from the highest down; the passes in between go through pool blocks that are handed back once enqueued.
static int32_t cmle_contract_passes(zk_ctx *c, const uint64_t *src, uint64_t m, const std::vector<uint32_t> &pos, const std::vector<Fe> &val,
                                    uint64_t *dst) {
    const FieldParams &P = c->fi->P;
    const size_t s = pos.size();
    PoolBlock hold[2];   // the source and the destination of the pass being enqueued, when they are intermediates
    for (size_t at = 0; at < s;) {
        const int G = s - at >= 3 ? 3 : (int)(s - at);
        CmleContract g;
        for (int i = 0; i < G; ++i) g.q[i] = pos[at + G - 1 - i];   // ascending inside the group
        for (int i = G; i < 3; ++i) g.q[i] = 0;
        for (int t = 0; t < 8; ++t) {
            Fe w = fe_one(P);
            for (int i = 0; i < G; ++i)
                if (t >> i & 1) w = fe_mul(w, val[at + G - 1 - i], P);
            g.w[t] = w;
        }
        const uint64_t m_out = m - G, n_out = 1ull << m_out;
        uint64_t *o = dst;
        PoolBlock next;
        if (at + G < s) {
            ZKCHK(next.alloc(c, mle_block_bytes(m_out)));
            o = next.as();
        }
        const uint32_t grid = cmle_stream_grid(n_out);
        if (G == 3) k_cmle_contract<3><<<grid, kBlock, 0, c->stream>>>(src, o, n_out, g, P);
        else if (G == 2) k_cmle_contract<2><<<grid, kBlock, 0, c->stream>>>(src, o, n_out, g, P);
        else k_cmle_contract<1><<<grid, kBlock, 0, c->stream>>>(src, o, n_out, g, P);
        HIPCHK(hipGetLastError());
        hold[0] = std::move(hold[1]);   // the block this pass read goes back (stream-ordered reuse), the one it wrote is the next source
        hold[1] = std::move(next);
        src = o;
        m = m_out;
        at += G;
    }
    return ZK_OK;
}
// partial_evaluate (:72-104) with get_variable_indexes' checks (:285-304), assignment by assignment in the caller's order
static int32_t cmle_partial_evaluate_impl(zk_ctx *c, const zk_cmle *p, const uint8_t *selectors, const uint64_t *selector_lens,
                                          const uint64_t *values, uint64_t n_assign, zk_cmle **out) {
    if (!c || !p || !out || (n_assign && (!selector_lens || !values))) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    uint64_t seen = p->fixed;
    std::vector<std::pair<uint32_t, Fe>> fresh;   // (compact position in p, value) of the variables this call fixes
    const uint8_t *sel = selectors;
    for (uint64_t i = 0; i < n_assign; ++i) {
        const uint64_t len = selector_lens[i];
        const uint8_t *mine = sel;
        if (len && !selectors) return ZK_ERR_BAD_ARG;
        sel += len;
        if (len > p->n_vars) continue;   // :87-89
        if (len != p->n_vars) return ZK_ERR_SELECTOR_LEN;
        uint64_t set = 0, v = 0;
        for (uint64_t b = 0; b < len; ++b)
            if (mine[b]) ++set, v = b;
        if (set != 1) return ZK_ERR_SELECTOR_SINGLE;
        if (seen >> v & 1) continue;   // no key has this bit any more (:93): the first assignment of a variable wins
        seen |= 1ull << v;
        const uint64_t below = ~p->fixed & ((1ull << v) - 1);
        fresh.emplace_back((uint32_t)__builtin_popcountll(below), fe_from_u64limbs(values + 4 * i));
    }
    ZKCHK(use_device(c));
    CmleHolder r;
    ZKCHK(cmle_alloc(c, p->n_vars, r.put(), seen));
    if (fresh.empty()) {
        HIPCHK(hipMemcpyAsync(r->d, p->d, (size_t)32 << p->log_len, hipMemcpyDeviceToDevice, c->stream));
    } else {
        std::sort(fresh.begin(), fresh.end(), [](const auto &x, const auto &y) { return x.first > y.first; });
        std::vector<uint32_t> pos;
        std::vector<Fe> val;
        for (const auto &f : fresh) pos.push_back(f.first), val.push_back(f.second);
        DrainOnExit drain(c);   // a failed call waits for the passes it enqueued before the result's block goes back
        ZKCHK(cmle_contract_passes(c, p->d, p->log_len, pos, val, r->d));
        drain.armed = false;
    }
    *out = r.release();
    return ZK_OK;
}
extern "C" int32_t zk_cmle_partial_evaluate(zk_ctx *c, const zk_cmle *p, const uint8_t *selectors, const uint64_t *selector_lens,
                                            const uint64_t *values, uint64_t n_assign, zk_cmle **out) {
    try {   // host vectors sized by the assignments: an allocation failure is a status, not an exception
        return cmle_partial_evaluate_impl(c, p, selectors, selector_lens, values, n_assign, out);
    } catch (const std::bad_alloc &) {
        return ZK_ERR_ALLOC;
    }
}
// relabel (:109-123): the presence vector of the keys {k : k & fixed == 0} is ~fixed whatever the coefficients are, and moving the
// present variables down in order maps key pdep(j, ~fixed) to key j: the same vector under a new name
extern "C" int32_t zk_cmle_relabel(zk_ctx *c, zk_cmle *p) {
    if (!c || !p) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    p->n_vars = p->log_len;
    p->fixed = 0;
    return ZK_OK;
}
extern "C" int32_t zk_cmle_scalar_multiply(zk_ctx *c, const zk_cmle *p, const uint64_t s[4], zk_cmle **out) {
    if (!c || !p || !s || !out) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    CmleHolder r;
    ZKCHK(cmle_alloc(c, p->n_vars, r.put(), p->fixed));
    const uint64_t n = 1ull << p->log_len;
    k_cmle_scale<<<cmle_stream_grid(n), kBlock, 0, c->stream>>>(p->d, r->d, n, fe_from_u64limbs(s), c->fi->P);
    HIPCHK(hipGetLastError());
    *out = r.release();
    return ZK_OK;
}
extern "C" int32_t zk_cmle_add(zk_ctx *c, const zk_cmle *a, const zk_cmle *b, zk_cmle **out) {
    if (!c || !a || !b || !out) return ZK_ERR_BAD_ARG;
    if (a->ctx != c || b->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (a->fixed || b->fixed) return ZK_ERR_UNSUPPORTED;   // the union of two masked key sets is no masked set: relabel first
    ZKCHK(use_device(c));
    const zk_cmle *longer = a->log_len > b->log_len ? a : b, *shorter = longer == a ? b : a;   // b on a tie (:360-365)
    CmleHolder r;
    ZKCHK(cmle_alloc(c, longer->n_vars, r.put()));
    const uint64_t n = 1ull << longer->log_len;
    k_cmle_add<<<cmle_stream_grid(n), kBlock, 0, c->stream>>>(longer->d, n, shorter->d, 1ull << shorter->log_len, r->d, c->fi->P);
    HIPCHK(hipGetLastError());
    *out = r.release();
    return ZK_OK;
}
extern "C" int32_t zk_cmle_mul(zk_ctx *c, const zk_cmle *a, const zk_cmle *b, zk_cmle **out) {
    if (!c || !a || !b || !out) return ZK_ERR_BAD_ARG;
    if (a->ctx != c || b->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (a->fixed || b->fixed) return ZK_ERR_UNSUPPORTED;
    if (a->n_vars + b->n_vars > kMaxVars) return ZK_ERR_UNSUPPORTED;   // before any allocation
    ZKCHK(use_device(c));
    CmleHolder r;
    ZKCHK(cmle_alloc(c, a->n_vars + b->n_vars, r.put()));
    const uint64_t n = 1ull << r->log_len;
    k_cmle_outer<<<cmle_stream_grid(n), kBlock, 0, c->stream>>>(a->d, (uint32_t)a->n_vars, b->d, n, r->d, c->fi->P);
    HIPCHK(hipGetLastError());
    *out = r.release();
    return ZK_OK;
}
// device time of the algebra calls, `reps` back-to-back calls between two HIP events (each call's result goes straight back to the pool,
// so every rep reuses the blocks of the warm-up call): op 0 = partial_evaluate of a, 1 = Add, 2 = scalar_multiply of a by values[0..4),
// 3 = Mul
static int32_t bench_cmle_algebra_impl(zk_ctx *c, int32_t op, const zk_cmle *a, const zk_cmle *b, const uint8_t *selectors,
                                       const uint64_t *selector_lens, const uint64_t *values, uint64_t n_assign, int32_t reps, double *out_ms) {
    if (!c || !out_ms || reps < 1 || op < 0 || op > 3 || !a) return ZK_ERR_BAD_ARG;
    if ((op == 1 || op == 3) && !b) return ZK_ERR_BAD_ARG;
    if (op == 2 && !values) return ZK_ERR_BAD_ARG;
    auto once = [&]() -> int32_t {
        CmleHolder r;
        if (op == 1) return zk_cmle_add(c, a, b, r.put());
        if (op == 2) return zk_cmle_scalar_multiply(c, a, values, r.put());
        if (op == 3) return zk_cmle_mul(c, a, b, r.put());
        return cmle_partial_evaluate_impl(c, a, selectors, selector_lens, values, n_assign, r.put());
    };
    // one warm call: pool blocks; argument and context errors end the call there
    return timed_span(c, 1, AfterWarm::kWait, reps, once, out_ms);
}
extern "C" int32_t zk_bench_cmle_algebra(zk_ctx *c, int32_t op, const zk_cmle *a, const zk_cmle *b, const uint8_t *selectors,
                                         const uint64_t *selector_lens, const uint64_t *values, uint64_t n_assign, int32_t reps, double *out_ms) {
    try {
        return bench_cmle_algebra_impl(c, op, a, b, selectors, selector_lens, values, n_assign, reps, out_ms);
    } catch (const std::bad_alloc &) {
        return ZK_ERR_ALLOC;
    }
}
