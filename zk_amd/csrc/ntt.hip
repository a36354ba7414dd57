// ntt.hip -- the fft crate's transform (fft/src/lib.rs:4-19) and UnivariatePolynomial (polynomial/src/univariate_poly.rs) of the C ABI:
// host side of ntt_kernels.cuh and upoly_kernels.cuh.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "ntt_kernels.cuh"
#include "upoly_kernels.cuh"

// ------------------------------------------------------------------------------------------------------------
// fft crate
// ------------------------------------------------------------------------------------------------------------
static int32_t make_twiddles(zk_ctx *c, uint32_t log_n, const Fe &omega, void **out, bool full = false) {
    const uint64_t count = full ? (1ull << log_n) : (log_n ? (1ull << (log_n - 1)) : 1);
    RawBlock tw;
    ZKCHK(raw_alloc(c, (size_t)count * 32, tw.put()));
    k_twiddle_table<<<grid_for((count + 63) / 64), kBlock, 0, c->stream>>>(static_cast<uint64_t *>(tw.get()), count, omega, c->fi->P);
    HIPCHK(hipGetLastError());
    *out = tw.release();   // the caller keeps it: the context's cache, or a RawBlock of its own
    return ZK_OK;
}
static int32_t ntt_with_table(zk_ctx *c, const uint64_t *in, uint64_t *out, uint32_t log_n, const uint64_t *tw) {
    const uint64_t n = 1ull << log_n;
    k_bitrev_copy<<<grid_for(n), kBlock, 0, c->stream>>>(in, out, log_n);
    HIPCHK(hipGetLastError());
    for (uint32_t s = 0; s < log_n; ++s) {
        k_ntt_stage<<<grid_for(n / 2), kBlock, 0, c->stream>>>(out, tw, log_n, s, c->fi->P);
        HIPCHK(hipGetLastError());
    }
    return ZK_OK;
}
// ---- LDS-staged multi-pass NTT (ntt_kernels.cuh) for n >= 2^8 ----
static void ntt_make_plan(uint32_t log_n, NttPlan &pl) {
    pl.log_n = log_n;
    pl.n_pass = (log_n + kNttMaxLog - 1) / kNttMaxLog;
    if (pl.n_pass < 2) pl.n_pass = 2;
    const uint32_t base = log_n / pl.n_pass, rem = log_n % pl.n_pass;
    for (uint32_t p = 0; p < 4; ++p) pl.l[p] = p < pl.n_pass ? base + (p < rem ? 1 : 0) : 0;
    pl.lo_bits = log_n < 12 ? log_n : 12;
    pl.w_lo = nullptr;
    pl.w_hi = nullptr;
    for (int p = 0; p < 4; ++p) pl.w_full[p] = nullptr;
}
static int32_t ntt_build_tables(zk_ctx *c, NttPlan &pl, const Fe &omega) {
    const uint32_t hi_bits = pl.log_n - pl.lo_bits;
    RawBlock lo_block, hi_block;
    ZKCHK(raw_alloc(c, ((size_t)kTw29Words * 4) << pl.lo_bits, lo_block.put()));
    ZKCHK(raw_alloc(c, (size_t)32 << hi_bits, hi_block.put()));
    uint32_t *lo = static_cast<uint32_t *>(lo_block.get());
    uint64_t *hi = static_cast<uint64_t *>(hi_block.get());
    k_ntt_tables<<<grid_for((1ull << pl.lo_bits) + (1ull << hi_bits)), kBlock, 0, c->stream>>>(lo, hi, pl.lo_bits, hi_bits, omega, c->fi->P);
    HIPCHK(hipGetLastError());
    pl.w_lo = static_cast<uint32_t *>(lo_block.release());   // the plan keeps them (the context's cache, or ntt_free_tables)
    pl.w_hi = static_cast<uint64_t *>(hi_block.release());
    // full inter-pass tables for the middle passes while they stay <= 2^24 entries (512 MiB): a 32-byte read per element instead
    // of the multiplication that composes the twiddle from the two-level table -- the passes are bound by VALU issue, not by HBM
    // (ZK_NTT_FULL_TABLE_MAX_LOG: largest table built, log2 entries; 0 = compose everything.  A/B: profiles/r05_ntt_table_ab.log)
    static const uint32_t full_max_log = (uint32_t)env_u64("ZK_NTT_FULL_TABLE_MAX_LOG", 24, 0, 24);
    uint32_t lo_sum = 0;
    for (uint32_t p = 0; p + 1 < pl.n_pass; ++p) {
        const uint32_t log_entries = pl.log_n - lo_sum;   // R_p * I_p = n / O_p
        if (log_entries <= full_max_log) {
            RawBlock t;   // optional: without it the pass composes its twiddles
            if (raw_alloc(c, (size_t)32 << log_entries, t.put()) == ZK_OK) {
                k_ntt_full_table<<<grid_for(1ull << log_entries), kBlock, 0, c->stream>>>(static_cast<uint64_t *>(t.get()), pl, log_entries - pl.l[p], pl.l[p],
                                                                                          lo_sum, c->fi->P);
                if (hipGetLastError() == hipSuccess) pl.w_full[p] = static_cast<uint64_t *>(t.release());
            }
        }
        lo_sum += pl.l[p];
    }
    return ZK_OK;
}
static void ntt_free_tables(NttPlan &pl) {
    if (pl.w_lo) (void)hipFree((void *)pl.w_lo);
    if (pl.w_hi) (void)hipFree((void *)pl.w_hi);
    for (int p = 0; p < 4; ++p)
        if (pl.w_full[p]) (void)hipFree((void *)pl.w_full[p]);
    pl.w_lo = nullptr;
    pl.w_hi = nullptr;
}
template <int L, bool LAST, int FUSE>
static hipError_t ntt_launch_lf(const NttPlan &pl, uint32_t p, uint32_t tiles, size_t lds, hipStream_t st, const uint64_t *src,
                                uint64_t *dst, const FieldParams &P, const Mul29 &scale, int do_scale, const NttFuseArgs &fz) {
    const hipError_t e =
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ntt_pass<L, LAST, FUSE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    k_ntt_pass<L, LAST, FUSE><<<tiles, kNttThreads, lds, st>>>(src, dst, pl, p, P, scale, do_scale, fz);
    return hipGetLastError();
}
// fuse: kNttPlain (zk_ntt), a first-pass / last-pass variant of the univariate product (zk_upoly_mul), or a batched variant of
// the interpolation's tree levels (zk_upoly_interpolate) and the multipoint evaluation's (zk_upoly_evaluate_many)
template <int L>
static hipError_t ntt_launch_l(const NttPlan &pl, uint32_t p, bool last, uint32_t tiles, size_t lds, hipStream_t st, const uint64_t *src,
                               uint64_t *dst, const FieldParams &P, const Mul29 &scale, int do_scale, int fuse, const NttFuseArgs &fz) {
    if (!last) {
        switch (fuse) {
            case kNttPlain: return ntt_launch_lf<L, false, kNttPlain>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
            case kNttPadLoad: return ntt_launch_lf<L, false, kNttPadLoad>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
            case kNttBatchPad: return ntt_launch_lf<L, false, kNttBatchPad>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
            case kNttBatch: return ntt_launch_lf<L, false, kNttBatch>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
            default: return hipErrorInvalidValue;
        }
    }
    switch (fuse) {
        case kNttPlain: return ntt_launch_lf<L, true, kNttPlain>(pl, p, tiles, lds, st, src, dst, P, scale, do_scale, fz);
        case kNttMulStore: return ntt_launch_lf<L, true, kNttMulStore>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
        case kNttSqrStore: return ntt_launch_lf<L, true, kNttSqrStore>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
        case kNttTruncStore: return ntt_launch_lf<L, true, kNttTruncStore>(pl, p, tiles, lds, st, src, dst, P, scale, 1, fz);
        case kNttBatch: return ntt_launch_lf<L, true, kNttBatch>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
        case kNttBatchCombine: return ntt_launch_lf<L, true, kNttBatchCombine>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
        case kNttBatchShift: return ntt_launch_lf<L, true, kNttBatchShift>(pl, p, tiles, lds, st, src, dst, P, scale, 1, fz);
        case kNttBatchMulAux: return ntt_launch_lf<L, true, kNttBatchMulAux>(pl, p, tiles, lds, st, src, dst, P, scale, 0, fz);
        case kNttBatchUpperAdd: return ntt_launch_lf<L, true, kNttBatchUpperAdd>(pl, p, tiles, lds, st, src, dst, P, scale, 1, fz);
        default: return hipErrorInvalidValue;
    }
}
static hipError_t ntt_launch_pass(const NttPlan &pl, uint32_t p, bool last, uint32_t tiles, size_t lds, hipStream_t st,
                                  const uint64_t *src, uint64_t *dst, const FieldParams &P, const Mul29 &scale, int do_scale,
                                  int fuse = kNttPlain, const NttFuseArgs &fz = NttFuseArgs{0}) {
    switch (pl.l[p]) {
        case 4: return ntt_launch_l<4>(pl, p, last, tiles, lds, st, src, dst, P, scale, do_scale, fuse, fz);
        case 5: return ntt_launch_l<5>(pl, p, last, tiles, lds, st, src, dst, P, scale, do_scale, fuse, fz);
        case 6: return ntt_launch_l<6>(pl, p, last, tiles, lds, st, src, dst, P, scale, do_scale, fuse, fz);
        case 7: return ntt_launch_l<7>(pl, p, last, tiles, lds, st, src, dst, P, scale, do_scale, fuse, fz);
        case 8: return ntt_launch_l<8>(pl, p, last, tiles, lds, st, src, dst, P, scale, do_scale, fuse, fz);
        default: return hipErrorInvalidValue;
    }
}
static Mul29 ntt_inverse_scale(const FieldParams &P, uint64_t n) {   // fft/src/lib.rs:17: * F::from(n).inverse()
    const uint64_t nl[4] = {n, 0, 0, 0};
    return mul29_prepare(fe_inverse(fe_from_canonical(fe_from_u64limbs(nl), P), P), P);
}
// the passes of one transform: the first one reads `in` (variant first_fuse), the middle ones run in place on `scratch` (n elements),
// the last one writes `out` (variant last_fuse)
static int32_t ntt_run_passes(zk_ctx *c, const NttPlan &pl, const uint64_t *in, uint64_t *out, uint64_t *scratch, bool inverse,
                              int first_fuse, const NttFuseArgs &first_fz, int last_fuse, const NttFuseArgs &last_fz) {
    const FieldParams &P = c->fi->P;
    const uint64_t n = 1ull << pl.log_n;
    const Mul29 scale = inverse ? ntt_inverse_scale(P, n) : Mul29{};
    const uint64_t *src = in;
    for (uint32_t p = 0; p < pl.n_pass; ++p) {
        const uint32_t R = 1u << pl.l[p];
        const size_t lds = (size_t)R * kNttRowBytes + (size_t)(R / 2) * kTw29Words * 4;   // one plane (halves take turns) + twiddles
        const uint32_t tiles = (uint32_t)(n / ((uint64_t)R * kNttCols));
        const bool last = p + 1 == pl.n_pass;
        const int fuse = last ? last_fuse : (p == 0 ? first_fuse : kNttPlain);
        hipError_t e = ntt_launch_pass(pl, p, last, tiles, lds, c->stream, src, last ? out : scratch, P, scale, (last && inverse) ? 1 : 0,
                                       fuse, last ? last_fz : first_fz);
        if (!last) src = scratch;   // middle passes keep their addresses: later ones run in place on scratch
        if (e != hipSuccess) {
            g_hip_err = std::string("ntt pass: ") + hipGetErrorString(e);
            return ZK_ERR_HIP;
        }
    }
    return ZK_OK;
}
// the passes of nb transforms of 2^log_n points at once (in, out and scratch hold transform t at t << log_n; kNttBatchPad reads its
// operand at t * in_stride + in_off): one launch per pass, the middle ones kNttBatch
static int32_t ntt_run_batched(zk_ctx *c, const NttPlan &pl, uint64_t nb, const uint64_t *in, uint64_t *out, uint64_t *scratch,
                               bool inverse, int first_fuse, const NttFuseArgs &first_fz, int last_fuse, const NttFuseArgs &last_fz) {
    const FieldParams &P = c->fi->P;
    const uint64_t n = 1ull << pl.log_n;
    const Mul29 scale = inverse ? ntt_inverse_scale(P, n) : Mul29{};
    const uint64_t *src = in;
    for (uint32_t p = 0; p < pl.n_pass; ++p) {
        const uint32_t R = 1u << pl.l[p];
        const size_t lds = (size_t)R * kNttRowBytes + (size_t)(R / 2) * kTw29Words * 4;
        const uint64_t tiles = nb * (n / ((uint64_t)R * kNttCols));
        if (tiles > 0x7fffffffull) return ZK_ERR_UNSUPPORTED;
        const bool last = p + 1 == pl.n_pass;
        const int fuse = last ? last_fuse : (p == 0 ? first_fuse : kNttBatch);
        hipError_t e = ntt_launch_pass(pl, p, last, (uint32_t)tiles, lds, c->stream, src, last ? out : scratch, P, scale, 0, fuse,
                                       last ? last_fz : (p == 0 ? first_fz : NttFuseArgs{0}));
        if (!last) src = scratch;
        if (e != hipSuccess) {
            g_hip_err = std::string("ntt batched pass: ") + hipGetErrorString(e);
            return ZK_ERR_HIP;
        }
    }
    return ZK_OK;
}
static int32_t ntt_run_plan(zk_ctx *c, const NttPlan &pl, const uint64_t *in, uint64_t *out, bool inverse) {
    const uint64_t n = 1ull << pl.log_n;
    PoolBlock scratch;
    ZKCHK(scratch.alloc(c, (size_t)n * 32));
    const NttFuseArgs none = {0};
    return ntt_run_passes(c, pl, in, out, scratch.as(), inverse, kNttPlain, none, kNttPlain, none);
}
// the context's cached plan + twiddle tables of the 2^log_n-point transform (log_n >= 8)
static int32_t ntt_cached_plan(zk_ctx *c, uint32_t log_n, bool inverse, const NttPlan **out) {
    const auto key = std::make_pair(log_n, inverse ? 1 : 0);
    auto pit = c->ntt_plans.find(key);
    if (pit == c->ntt_plans.end()) {
        Fe omega;
        if (!field_root_of_unity(*c->fi, log_n, omega)) return ZK_ERR_FFT_NO_ROOT;
        if (inverse) omega = fe_inverse(omega, c->fi->P);
        NttPlan pl;
        ntt_make_plan(log_n, pl);
        ZKCHK(ntt_build_tables(c, pl, omega));
        pit = c->ntt_plans.emplace(key, pl).first;
    }
    *out = &pit->second;
    return ZK_OK;
}

extern "C" int32_t zk_ntt(zk_ctx *c, const zk_mle *in, int32_t inverse, zk_mle *out) {
    if (!c || !in || !out) return ZK_ERR_BAD_ARG;
    if (in->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (in->n_vars != out->n_vars || in->d == out->d) return ZK_ERR_BAD_ARG;
    const uint32_t log_n = (uint32_t)in->n_vars;
    Fe omega;
    if (!field_root_of_unity(*c->fi, log_n, omega)) return ZK_ERR_FFT_NO_ROOT;   // fft/src/lib.rs:6
    ZKCHK(use_device(c));
    const FieldParams &P = c->fi->P;
    if (inverse) omega = fe_inverse(omega, P);                                   // fft/src/lib.rs:14
    auto key = std::make_pair(log_n, inverse ? 1 : 0);
    if (log_n >= 8) {
        auto pit = c->ntt_plans.find(key);
        if (pit == c->ntt_plans.end()) {
            NttPlan pl;
            ntt_make_plan(log_n, pl);
            ZKCHK(ntt_build_tables(c, pl, omega));
            pit = c->ntt_plans.emplace(key, pl).first;
        }
        return ntt_run_plan(c, pit->second, in->d, out->d, inverse != 0);
    }
    auto it = c->twiddles.find(key);
    if (it == c->twiddles.end()) {
        void *tw = nullptr;
        ZKCHK(make_twiddles(c, log_n, omega, &tw));
        it = c->twiddles.emplace(key, static_cast<uint64_t *>(tw)).first;
    }
    ZKCHK(ntt_with_table(c, in->d, out->d, log_n, it->second));
    if (inverse) {                                                               // fft/src/lib.rs:17
        const uint64_t nl[4] = {1ull << log_n, 0, 0, 0};                         // F::from(n).inverse()
        const Fe ninv = fe_inverse(fe_from_canonical(fe_from_u64limbs(nl), P), P);
        k_scale<<<grid_for(1ull << log_n), kBlock, 0, c->stream>>>(out->d, 1ull << log_n, ninv, P);
        HIPCHK(hipGetLastError());
    }
    return ZK_OK;
}
static int32_t fft_host_common(zk_ctx *c, const uint64_t *in, uint64_t n, uint64_t *out, int mode, const uint64_t *omega_user) {
    if (!c || !out || (!in && n)) return ZK_ERR_BAD_ARG;
    if (mode == 2) {                                        // fft_internal: len 1 returns, non power of two panics (:22-30)
        if (n == 0 || (n & (n - 1))) return ZK_ERR_FFT_NOT_POW2;
    } else {                                                // fft / ifft: get_root_of_unity(n) first (:6, :14)
        if (n == 0 || (n & (n - 1))) return ZK_ERR_FFT_NO_ROOT;
    }
    uint32_t log_n = 0;
    while ((1ull << log_n) < n) ++log_n;
    if (mode != 2 && log_n > c->fi->two_adicity) return ZK_ERR_FFT_NO_ROOT;
    if (log_n > kMaxVars) return ZK_ERR_UNSUPPORTED;
    MleHolder a, b;
    ZKCHK(zk_mle_upload(c, log_n, in, n, a.put()));
    ZKCHK(mle_alloc(c, log_n, b.put()));
    {
        // every other path uses the (u + t, u - t) butterfly, i.e. assumes omega^(n/2) = -1; fft_internal's caller may pass
        // any omega (fft/src/lib.rs:21), for which the reference's literal omega^(i + n/2) differs: full-table stages
        bool primitive = true;
        if (mode == 2 && log_n >= 1) {
            const FieldParams &P = c->fi->P;
            primitive = fe_eq(fe_pow_u64(fe_from_u64limbs(omega_user), n / 2, P), fe_sub(fe_zero(), fe_one(P), P));
        }
        // the caller's omega has no cached tables: they live for this call (hipFree waits for the device)
        if (mode == 2 && !primitive) {
            RawBlock tw;
            ZKCHK(make_twiddles(c, log_n, fe_from_u64limbs(omega_user), tw.put(), /*full=*/true));
            k_bitrev_copy<<<grid_for(n), kBlock, 0, c->stream>>>(a->d, b->d, log_n);
            for (uint32_t s = 0; s < log_n; ++s)
                k_ntt_stage_generic<<<grid_for(n / 2), kBlock, 0, c->stream>>>(b->d, static_cast<const uint64_t *>(tw.get()), log_n, s, c->fi->P);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(c->stream));
        } else if (mode == 2 && log_n >= 8) {
            NttPlan pl;
            ntt_make_plan(log_n, pl);
            struct PlanTables {   // frees what ntt_build_tables got as far as building
                NttPlan &pl;
                ~PlanTables() { ntt_free_tables(pl); }
            } tables{pl};
            ZKCHK(ntt_build_tables(c, pl, fe_from_u64limbs(omega_user)));
            DrainOnExit drain(c);
            ZKCHK(ntt_run_plan(c, pl, a->d, b->d, false));
            ZKCHK(drain.wait());
        } else if (mode == 2) {
            RawBlock tw;
            ZKCHK(make_twiddles(c, log_n, fe_from_u64limbs(omega_user), tw.put()));
            DrainOnExit drain(c);
            ZKCHK(ntt_with_table(c, a->d, b->d, log_n, static_cast<const uint64_t *>(tw.get())));
            ZKCHK(drain.wait());
        } else {
            ZKCHK(zk_ntt(c, a.get(), mode, b.get()));
        }
    }
    return zk_mle_download(c, b.get(), out);
}
extern "C" int32_t zk_fft_host(zk_ctx *c, const uint64_t *in, uint64_t n, uint64_t *out) { return fft_host_common(c, in, n, out, 0, nullptr); }
extern "C" int32_t zk_ifft_host(zk_ctx *c, const uint64_t *in, uint64_t n, uint64_t *out) { return fft_host_common(c, in, n, out, 1, nullptr); }
extern "C" int32_t zk_fft_internal_host(zk_ctx *c, const uint64_t *in, uint64_t n, const uint64_t omega[4], uint64_t *out) {
    if (!omega) return ZK_ERR_BAD_ARG;
    return fft_host_common(c, in, n, out, 2, omega);
}

// ------------------------------------------------------------------------------------------------------------
// UnivariatePolynomial (polynomial/src/univariate_poly.rs): ::new, ::coefficients, ::evaluate, Mul.  DESIGN.md section 11.
// ------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kUpolyMaxLog = 32;   // largest planned transform (four passes of <= 2^8)
static uint32_t ceil_log2_u64(uint64_t v) {
    uint32_t l = 0;
    while (l < 64 && (1ull << l) < v) ++l;
    return l;
}
static size_t upoly_block_bytes(uint64_t len) { return (size_t)32 << ceil_log2_u64(len ? len : 1); }
int32_t zk::upoly_alloc(zk_ctx *c, uint64_t len, zk_upoly **out) {
    if (len > (1ull << kMaxVars)) return ZK_ERR_UNSUPPORTED;
    zk_upoly *p = new (std::nothrow) zk_upoly();
    if (!p) return ZK_ERR_ALLOC;
    p->ctx = c;
    p->len = len;
    PoolBlock blk;
    const int32_t rc = blk.alloc(c, upoly_block_bytes(len));
    if (rc != ZK_OK) {
        delete p;
        return rc;
    }
    p->d = static_cast<uint64_t *>(blk.release());   // the handle owns the block from here on (upoly_release)
    *out = p;
    return ZK_OK;
}
void zk::upoly_release(zk_upoly *p) {
    if (!p) return;
    pool_free(p->ctx, p->d, upoly_block_bytes(p->len));
    delete p;
}
extern "C" int32_t zk_upoly_upload(zk_ctx *c, const uint64_t *coeffs, uint64_t len, zk_upoly **out) {
    if (!c || !out || (!coeffs && len)) return ZK_ERR_BAD_ARG;
    ZKCHK(use_device(c));
    UpolyHolder p;
    ZKCHK(upoly_alloc(c, len, p.put()));
    if (len) {
        hipError_t e = hipMemcpyAsync(p->d, coeffs, (size_t)len * 32, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            g_hip_err = std::string("upload: ") + hipGetErrorString(e);
            return ZK_ERR_HIP;
        }
    }
    *out = p.release();
    return ZK_OK;
}
extern "C" int32_t zk_upoly_len(const zk_upoly *p, uint64_t *out_len) {
    if (!p || !out_len) return ZK_ERR_BAD_ARG;
    *out_len = p->len;
    return ZK_OK;
}
extern "C" int32_t zk_upoly_download(zk_ctx *c, const zk_upoly *p, uint64_t *out) {
    if (!c || !p || (!out && p->len)) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (!p->len) return ZK_OK;
    ZKCHK(use_device(c));
    HIPCHK(hipMemcpyAsync(out, p->d, (size_t)p->len * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
extern "C" int32_t zk_upoly_free(zk_ctx *c, zk_upoly *p) {
    if (!p) return ZK_OK;
    if (!c) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    upoly_release(p);   // back to the context's pool; reuse is stream-ordered
    return ZK_OK;
}
// product length la + lb - 1 (both > 0) -> log2 of the padded transform; ZK_ERR_UNSUPPORTED past the field's two-adicity,
// kMaxVars or the largest planned transform
static int32_t upoly_product_log(const zk_ctx *c, uint64_t la, uint64_t lb, uint32_t *out_log) {
    if (la > (1ull << kMaxVars) || lb > (1ull << kMaxVars)) return ZK_ERR_UNSUPPORTED;
    const uint32_t log_n = ceil_log2_u64(la + lb - 1);
    if (log_n > c->fi->two_adicity || log_n > kMaxVars || log_n > kUpolyMaxLog) return ZK_ERR_UNSUPPORTED;
    *out_log = log_n;
    return ZK_OK;
}
// Direct convolution or NTT.  Below the LDS-staged NTT's 2^8 points always direct; otherwise, with ZK_UPOLY_DIRECT_MAX set, direct iff
// min(la, lb) <= its value, and unset, by a cost model fitted to the crossover measured on the MI355X (profiles/upoly.log, DESIGN.md
// section 11): the direct kernel takes max(0.7 us per coefficient of the shorter operand -- one thread's serial chain --, 9 ps per
// product at throughput), the three transforms 95 us + 0.35 ns per output coefficient.
static constexpr uint64_t kUpolyModel = ~0ull;
static bool upoly_direct(uint64_t la, uint64_t lb, uint32_t log_n) {
    static const uint64_t forced = env_u64("ZK_UPOLY_DIRECT_MAX", kUpolyModel, 0, 1ull << 40);
    const uint64_t m = std::min(la, lb);
    if (log_n < 8) return true;
    if (forced != kUpolyModel) return m <= forced;
    const double total = (double)(la + lb), direct_us = std::max(0.7 * (double)m, 9e-6 * (double)m * total), ntt_us = 95.0 + 3.5e-4 * total;
    return direct_us <= ntt_us;
}
// out (>= la + lb - 1 elements) = a * b; a == b (same buffer and length) squares.  Asynchronous.
static int32_t upoly_mul_into(zk_ctx *c, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, uint64_t *out, uint32_t log_n) {
    const uint64_t lc = la + lb - 1;
    if (upoly_direct(la, lb, log_n)) {
        const bool a_short = la <= lb;
        uint64_t g = (lc + kBlock - 1) / kBlock;
        if (g > kMaxGridStream) g = kMaxGridStream;
        k_upoly_direct<<<(uint32_t)g, kBlock, 0, c->stream>>>(a_short ? a : b, a_short ? la : lb, a_short ? b : a, a_short ? lb : la, out,
                                                               c->fi->P);
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    // NTT path: NTT(a) -> T, NTT(b) with T multiplied in on the store -> T, INTT(T) truncated into out: 3 x n_pass launches (a
    // square: 2 x n_pass).  T and the transforms' scratch come from the pool.
    const NttPlan *fw = nullptr, *inv = nullptr;
    ZKCHK(ntt_cached_plan(c, log_n, false, &fw));
    ZKCHK(ntt_cached_plan(c, log_n, true, &inv));
    const size_t bytes = (size_t)32 << log_n;
    PoolScope ps(c);
    uint64_t *t = nullptr, *scratch = nullptr;
    ZKCHK(ps.get(bytes, &t));
    ZKCHK(ps.get(bytes, &scratch));
    const NttFuseArgs none = {0};
    if (a == b && la == lb) {
        ZKCHK(ntt_run_passes(c, *fw, a, t, scratch, false, kNttPadLoad, NttFuseArgs{la}, kNttSqrStore, none));
    } else {
        ZKCHK(ntt_run_passes(c, *fw, a, t, scratch, false, kNttPadLoad, NttFuseArgs{la}, kNttPlain, none));
        ZKCHK(ntt_run_passes(c, *fw, b, t, scratch, false, kNttPadLoad, NttFuseArgs{lb}, kNttMulStore, none));
    }
    return ntt_run_passes(c, *inv, t, out, scratch, true, kNttPlain, none, kNttTruncStore, NttFuseArgs{lc});
}
extern "C" int32_t zk_upoly_mul(zk_ctx *c, const zk_upoly *a, const zk_upoly *b, zk_upoly **out) {
    if (!c || !a || !b || !out) return ZK_ERR_BAD_ARG;
    if (a->ctx != c || b->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    if (a->len == 0 || b->len == 0) return upoly_alloc(c, 0, out);   // univariate_poly.rs:190-192
    uint32_t log_n = 0;
    ZKCHK(upoly_product_log(c, a->len, b->len, &log_n));
    UpolyHolder o;
    ZKCHK(upoly_alloc(c, a->len + b->len - 1, o.put()));
    ZKCHK(upoly_mul_into(c, a->d, a->len, b->d, b->len, o->d, log_n));
    *out = o.release();
    return ZK_OK;
}
extern "C" int32_t zk_upoly_mul_host(zk_ctx *c, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, uint64_t *out) {
    if (!c || (!a && la) || (!b && lb)) return ZK_ERR_BAD_ARG;
    if (la == 0 || lb == 0) return ZK_OK;   // empty product: nothing is written
    if (!out) return ZK_ERR_BAD_ARG;
    uint32_t log_n = 0;
    ZKCHK(upoly_product_log(c, la, lb, &log_n));   // before anything is read or allocated
    UpolyHolder pa, pb, pc;
    ZKCHK(zk_upoly_upload(c, a, la, pa.put()));
    if (a != b || la != lb) ZKCHK(zk_upoly_upload(c, b, lb, pb.put()));
    ZKCHK(zk_upoly_mul(c, pa.get(), pb.get() ? pb.get() : pa.get(), pc.put()));
    return zk_upoly_download(c, pc.get(), out);
}
// ::evaluate (univariate_poly.rs:29-40): Horner there, a sum of c[i] x^i here (field addition is exact: same bits).  Three launches
// (power table, block sums, final sum) and one host wait.
extern "C" int32_t zk_upoly_evaluate(zk_ctx *c, const zk_upoly *p, const uint64_t x[4], uint64_t out[4]) {
    if (!c || !p || !x || !out) return ZK_ERR_BAD_ARG;
    if (p->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (p->len == 0) {   // an empty fold: F::zero()
        for (int i = 0; i < 4; ++i) out[i] = 0;
        return ZK_OK;
    }
    ZKCHK(use_device(c));
    const FieldParams &P = c->fi->P;
    const uint32_t lo_bits = std::min<uint32_t>(12, ceil_log2_u64(p->len));
    const uint64_t n_hi = (p->len + (1ull << lo_bits) - 1) >> lo_bits, n_tab = (1ull << lo_bits) + n_hi;
    const size_t tab_bytes = (size_t)n_tab * kTw29Words * 4;
    PoolBlock tab_block;   // goes back once its readers are enqueued: stream-ordered reuse
    ZKCHK(tab_block.alloc(c, tab_bytes));
    uint32_t *tab = tab_block.as<uint32_t>();
    uint32_t *hi = tab + ((size_t)kTw29Words << lo_bits);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_hi, kMaxGrid);   // d_partials holds kMaxGrid * kMaxSums elements
    k_upoly_powers<<<grid_for(n_tab), kBlock, 0, c->stream>>>(tab, hi, lo_bits, n_hi, fe_from_u64limbs(x), P);
    k_upoly_eval<<<grid, kBlock, 0, c->stream>>>(p->d, p->len, tab, hi, lo_bits, P, c->d_partials);
    k_upoly_eval_final<<<1, kBlock, 0, c->stream>>>(c->d_partials, grid, P, c->d_sums);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_pinned, c->d_sums, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 4; ++i) out[i] = c->h_pinned[i];
    return ZK_OK;
}

// Add for &UnivariatePolynomial (univariate_poly.rs:157-184).  Asynchronous.
static int32_t upoly_add_into(zk_ctx *c, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, uint64_t *out) {
    const uint64_t n = std::max(la, lb);
    if (!n) return ZK_OK;
    k_upoly_add<<<grid_for(n), kBlock, 0, c->stream>>>(a, la, b, lb, out, c->fi->P);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
extern "C" int32_t zk_upoly_add(zk_ctx *c, const zk_upoly *a, const zk_upoly *b, zk_upoly **out) {
    if (!c || !a || !b || !out) return ZK_ERR_BAD_ARG;
    if (a->ctx != c || b->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(use_device(c));
    UpolyHolder o;
    ZKCHK(upoly_alloc(c, std::max(a->len, b->len), o.put()));
    ZKCHK(upoly_add_into(c, a->d, a->len, b->d, b->len, o->d));
    *out = o.release();
    return ZK_OK;
}

// ---- interpolation --------------------------------------------------------------------------------
// n points -> log2 of the largest transform the tree and the merges run (2^ceil(log2 n) points); ZK_ERR_UNSUPPORTED past the
// field's two-adicity, kMaxVars or the largest planned transform.  Checked before anything is read or allocated.
static int32_t upoly_interp_log(const zk_ctx *c, uint64_t n, uint32_t *out_log) {
    if (n > (1ull << kMaxVars)) return ZK_ERR_UNSUPPORTED;
    const uint32_t log_n = ceil_log2_u64(n);
    if (log_n > c->fi->two_adicity || log_n > kUpolyMaxLog) return ZK_ERR_UNSUPPORTED;
    *out_log = log_n;
    return ZK_OK;
}
// exclusive product scan (k_scan_prod_*): out[i] = prod over k < i (rev = 0) or k > i (rev = 1) of v[k] (v null: F::from(max(k, 1)));
// *total_at gets a device pointer to the product of all n values
static int32_t upoly_scan_prod(zk_ctx *c, PoolScope &ps, const uint64_t *v, uint64_t n, int rev, uint64_t *out, const uint64_t **total_at) {
    const uint64_t nc = (n + kScanChunk - 1) / kScanChunk;
    if (nc > 0xffffffffull) return ZK_ERR_UNSUPPORTED;
    uint64_t *tot = nullptr;
    ZKCHK(ps.get(upoly_block_bytes(nc + 1), &tot));
    k_scan_prod_partial<<<(uint32_t)nc, kBlock, 0, c->stream>>>(v, n, rev, c->fi->P, tot);
    k_scan_prod_totals<<<1, kBlock, 0, c->stream>>>(tot, (uint32_t)nc, c->fi->P);
    k_scan_prod_apply<<<(uint32_t)nc, kBlock, 0, c->stream>>>(v, n, rev, c->fi->P, tot, out);
    HIPCHK(hipGetLastError());
    *total_at = tot + 4 * nc;
    return ZK_OK;
}
// Direct tree levels below 2^ZK_UPOLY_INTERP_DIRECT_LOG points per node, batched NTT levels above (the NTT's smallest transform is
// 2^8 points: nodes of 2^7 and more).  7 measured faster than 8 on the MI355X (profiles/upoly_interp.log).
static uint32_t upoly_interp_direct_log() {
    static const uint32_t d = (uint32_t)env_u64("ZK_UPOLY_INTERP_DIRECT_LOG", 7, 7, 8);
    return d;
}
static int32_t upoly_tree_direct(zk_ctx *c, uint32_t D, const uint64_t *w, const uint64_t *xs, uint64_t n, uint64_t *mo, uint64_t *po) {
    const uint64_t chunks = (n + (1ull << D) - 1) >> D;
    if (chunks > 0x7fffffffull) return ZK_ERR_UNSUPPORTED;
    if (D == 8) k_interp_tree_direct<8><<<(uint32_t)chunks, 256, 0, c->stream>>>(w, xs, n, c->fi->P, mo, po);
    else k_interp_tree_direct<7><<<(uint32_t)chunks, 128, 0, c->stream>>>(w, xs, n, c->fi->P, mo, po);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// Timing split for tools/upoly_interp_bench.py (zk_bench_upoly_interp), mk: marks after the weights (0), the direct levels (1) and the NTT
// levels (2).
// out (n elements) = sum_i w_i M(x) / (x - x_i) over the n points (xs null: x_i = i), w in W (n elements, consumed).  Asynchronous.
static int32_t upoly_interp_tree(zk_ctx *c, PoolScope &ps, const uint64_t *W, const uint64_t *xs, uint64_t n, uint64_t *out,
                                 const PhaseEvents *mk) {
    const uint32_t D = upoly_interp_direct_log();
    const bool pow2 = (n & (n - 1)) == 0;
    const uint32_t top = ceil_log2_u64(n + 1) - 1;   // the largest block: 2^top
    // buffers: m[2], p[2] ping-pong between levels; with n a power of two the root's P lands in `out` directly
    uint64_t *mb[2] = {nullptr, nullptr}, *pb[2] = {nullptr, nullptr};
    ZKCHK(ps.get(upoly_block_bytes(n), &mb[0]));
    if (top > D) ZKCHK(ps.get(upoly_block_bytes(n), &mb[1]));
    const uint32_t root_par = top > D ? (top - D) & 1 : 0;
    for (int q = 0; q < 2; ++q) {
        if (pow2 && (uint32_t)q == root_par) pb[q] = out;
        else if (q == 0 || top > D) ZKCHK(ps.get(upoly_block_bytes(n), &pb[q]));
    }
    ZKCHK(upoly_tree_direct(c, D, W, xs, n, mb[0], pb[0]));
    if (mk) ZKCHK(mk->mark(1));
    // batched NTT levels: level l combines the n >> (l + 1) nodes of 2^(l+1) points of the prefix; 4 forward transforms (pad on load,
    // the fourth one combining), 2 inverse (shift on store); the root of a power-of-two n needs no m
    if (top > D) {
        uint64_t *T[3] = {nullptr, nullptr, nullptr}, *S = nullptr;
        for (int q = 0; q < 3; ++q) ZKCHK(ps.get(upoly_block_bytes(n), &T[q]));
        ZKCHK(ps.get(upoly_block_bytes(n), &S));
        uint32_t cur = 0;
        for (uint32_t l = D; (n >> (l + 1)) != 0; ++l, cur ^= 1) {
            const uint64_t nb = n >> (l + 1), s = 1ull << l;
            const NttPlan *fw = nullptr, *iv = nullptr;
            ZKCHK(ntt_cached_plan(c, l + 1, false, &fw));
            ZKCHK(ntt_cached_plan(c, l + 1, true, &iv));
            const uint64_t *mc = mb[cur], *pc = pb[cur];
            const NttFuseArgs none = {0};
            const NttFuseArgs left = {s, 2 * s, 0, nullptr, nullptr}, right = {s, 2 * s, s, nullptr, nullptr};
            const NttFuseArgs comb = {0, 0, 0, T[1], T[2]};
            ZKCHK(ntt_run_batched(c, *fw, nb, mc, T[0], S, false, kNttBatchPad, left, kNttBatch, none));
            ZKCHK(ntt_run_batched(c, *fw, nb, mc, T[1], S, false, kNttBatchPad, right, kNttBatch, none));
            ZKCHK(ntt_run_batched(c, *fw, nb, pc, T[2], S, false, kNttBatchPad, left, kNttBatch, none));
            ZKCHK(ntt_run_batched(c, *fw, nb, pc, T[0], S, false, kNttBatchPad, right, kNttBatchCombine, comb));
            if (!(pow2 && nb == 1))
                ZKCHK(ntt_run_batched(c, *iv, nb, T[0], mb[cur ^ 1], S, true, kNttBatch, none, kNttBatchShift,
                                      NttFuseArgs{0, 0, 0, const_cast<uint64_t *>(mc), nullptr}));
            ZKCHK(ntt_run_batched(c, *iv, nb, T[1], pb[cur ^ 1], S, true, kNttBatch, none, kNttBatchShift,
                                  NttFuseArgs{0, 0, 0, const_cast<uint64_t *>(pc), nullptr}));
        }
    }
    if (mk) ZKCHK(mk->mark(2));
    if (pow2) return ZK_OK;
    // block merges, smallest block first: T (the blocks merged so far, t points) with the next larger block A to its left
    std::vector<uint32_t> bits;
    for (int b = 63; b >= 0; --b)
        if ((n >> b) & 1) bits.push_back((uint32_t)b);
    auto par = [&](uint32_t b) { return b > D ? (b - D) & 1 : 0u; };
    uint64_t start = n;
    std::vector<uint64_t> starts(bits.size());
    for (size_t j = bits.size(); j-- > 0;) starts[j] = (start -= 1ull << bits[j]);
    const uint32_t last_b = bits.back();
    const uint64_t *tm = mb[par(last_b)] + 4 * starts.back(), *tp = pb[par(last_b)] + 4 * starts.back();
    uint64_t t = 1ull << last_b;
    uint64_t *mm = nullptr, *pm = nullptr, *mp = nullptr, *acc_m[2] = {nullptr, nullptr}, *acc_p[2] = {nullptr, nullptr};
    ZKCHK(ps.get(upoly_block_bytes(n), &mm));
    ZKCHK(ps.get(upoly_block_bytes(n), &pm));
    ZKCHK(ps.get(upoly_block_bytes(n), &mp));
    if (bits.size() > 2)
        for (int q = 0; q < 2; ++q) {
            ZKCHK(ps.get(upoly_block_bytes(n), &acc_m[q]));
            ZKCHK(ps.get(upoly_block_bytes(n), &acc_p[q]));
        }
    for (size_t j = bits.size() - 1, q = 0; j-- > 0; q ^= 1) {
        const uint64_t a = 1ull << bits[j];
        const uint64_t *ma = mb[par(bits[j])] + 4 * starts[j], *pa = pb[par(bits[j])] + 4 * starts[j];
        const bool final_merge = j == 0;
        uint32_t lg = 0;
        ZKCHK(upoly_product_log(c, a, t, &lg));
        if (!final_merge) ZKCHK(upoly_mul_into(c, ma, a, tm, t, mm, lg));
        ZKCHK(upoly_mul_into(c, pa, a, tm, t, pm, lg));
        ZKCHK(upoly_mul_into(c, tp, t, ma, a, mp, lg));
        uint64_t *om = final_merge ? nullptr : acc_m[q], *op = final_merge ? out : acc_p[q];
        k_interp_merge<<<grid_for(a + t), kBlock, 0, c->stream>>>(ma, pa, a, tm, tp, t, final_merge ? nullptr : mm, pm, mp, c->fi->P, om, op);
        HIPCHK(hipGetLastError());
        tm = om;
        tp = op;
        t += a;
    }
    return ZK_OK;
}
// ---- series inverse ------------------------------------------------------------------------------------
// The length rule of the Newton inversion to k >= 1 coefficients, K = 2^ceil(log2 k): its largest products are 2t x t at t = K/2
// and (the division's) k x k, both 2K-point transforms, so it is available when 2K <= 2^min(two_adicity, kUpolyMaxLog).
static int32_t upoly_series_log(const zk_ctx *c, uint64_t k, uint32_t *out_log) {
    if (k > (1ull << kMaxVars)) return ZK_ERR_UNSUPPORTED;
    const uint32_t log_K = ceil_log2_u64(k);
    if (log_K + 1 > std::min<uint32_t>(c->fi->two_adicity, kUpolyMaxLog)) return ZK_ERR_UNSUPPORTED;
    *out_log = log_K;
    return ZK_OK;
}
// out (k >= 1 elements) = 1 / f mod z^k for f of lf >= 1 coefficients (the ones beyond lf count as 0), by Newton steps on the
// univariate product: alpha <- alpha (2 - f alpha) mod z^min(2t, k), each product over the coefficients that exist (f is never
// padded).  f[0] is inverted on the device and *flag |= 1 when it is 0 (the result is then all zeros); flag null: f[0] = 1 by
// construction and nothing is inverted.  Asynchronous.
static int32_t upoly_inverse_series_into(zk_ctx *c, const uint64_t *f, uint64_t lf, uint64_t k, uint64_t *out, uint32_t *flag) {
    const FieldParams &P = c->fi->P;
    const uint64_t K = 1ull << ceil_log2_u64(k);
    PoolScope ps(c);
    uint64_t *al[2] = {out, nullptr}, *e = nullptr, *g = nullptr;
    if (k > 1) {
        for (int q = 0; q < 2; ++q) ZKCHK(ps.get(upoly_block_bytes(2 * K), &al[q]));
        ZKCHK(ps.get(upoly_block_bytes(2 * K), &e));
        ZKCHK(ps.get(upoly_block_bytes(K), &g));
    }
    if (flag) k_fe_invert_checked<<<1, 64, 0, c->stream>>>(f, al[0], P, flag);
    else k_fe_fill_one<<<1, kBlock, 0, c->stream>>>(al[0], 1, P);
    HIPCHK(hipGetLastError());
    if (k == 1) return ZK_OK;
    uint32_t cur = 0;
    for (uint64_t t = 1; t < k; t <<= 1, cur ^= 1) {
        const uint64_t n2 = std::min(2 * t, k), fl = std::min(lf, n2);
        uint32_t lg = 0;
        ZKCHK(upoly_product_log(c, fl, t, &lg));
        ZKCHK(upoly_mul_into(c, f, fl, al[cur], t, e, lg));
        k_evalmany_two_minus<<<grid_for(n2), kBlock, 0, c->stream>>>(e, fl + t - 1, n2, P, g);
        HIPCHK(hipGetLastError());
        ZKCHK(upoly_product_log(c, t, n2, &lg));
        ZKCHK(upoly_mul_into(c, al[cur], t, g, n2, al[cur ^ 1], lg));   // t + n2 - 1 coefficients, the first n2 are alpha's
    }
    k_evalmany_pad<<<grid_for(k), kBlock, 0, c->stream>>>(al[cur], k, k, out);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// ---- multipoint evaluation ---------------------------------------------------------------------------
// The length rule of zk_upoly_evaluate_many, checked before anything is read or allocated: N = 2^ceil(log2 max(n, L, 1)); the tree
// path's largest transform is 2N points, so it is available when 2N <= 2^min(two_adicity, kUpolyMaxLog); without it the direct
// path runs up to n L = 2^40 products (about 12 s at the measured 9e10 modmul/s), ZK_ERR_UNSUPPORTED past that.
static constexpr uint64_t kEvalManyDirectCap = 1ull << 40;
struct EvalManyShape {
    uint32_t log_N;
    bool tree_ok;
    uint64_t products;   // n L, saturated at 2^40 + 1
};
static int32_t upoly_evalmany_shape(const zk_ctx *c, uint64_t L, uint64_t n, EvalManyShape *sh) {
    sh->log_N = ceil_log2_u64(std::max<uint64_t>(std::max(n, L), 1));
    sh->tree_ok = sh->log_N + 1 <= std::min<uint32_t>(c->fi->two_adicity, kUpolyMaxLog);
    sh->products = (L && n > kEvalManyDirectCap / L) ? kEvalManyDirectCap + 1 : n * L;
    if (!sh->tree_ok && sh->products > kEvalManyDirectCap) return ZK_ERR_UNSUPPORTED;
    return ZK_OK;
}
// Direct or tree.  With ZK_UPOLY_EVALMANY_DIRECT_MAX set, direct iff n L <= its value (0: always the tree where it is available);
// unset, by a cost model fitted to profiles/upoly_evalmany.log (MI355X, BN254).  The direct kernel takes the
// larger of its serial chain, 0.65 us per coefficient of a lane's chunk (0.67 ms for 2^10 coefficients in one chunk), and of its
// n L products at 1.2e5 per us (1.04e11 .. 1.24e11 modmul/s measured from 2^14 up); the tree 20 log2(N)^2 + 0.024 N us (measured
// 1.8 / 4.1 / 10.0 / 26 / 437 ms at N = 2^10 / 2^14 / 2^18 / 2^20 / 2^24, the formula within 30 % of each).  n = L crosses between
// 2^14 (direct 2.6 ms, tree 4.1) and 2^16 (35 against 6.0); both lopsided shapes of the log go direct, as measured.
static constexpr double kEvalManyChainUs = 0.65, kEvalManyDirectRate = 1.2e5, kEvalManyTreeLog2Us = 20.0, kEvalManyTreePerPoint = 0.024;
static constexpr uint64_t kEvalManyChunkMin = 1024, kEvalManyBlocksWanted = 1024;
// the direct path's split of the coefficients: chunks of *chunk coefficients on the grid's second axis
static uint32_t upoly_evalmany_chunks(uint64_t L, uint64_t n, uint64_t *chunk) {
    const uint64_t tiles = (n + kBlock - 1) / kBlock;
    uint64_t want = tiles >= kEvalManyBlocksWanted ? 1 : (kEvalManyBlocksWanted + tiles - 1) / tiles;
    want = std::min<uint64_t>(want, std::max<uint64_t>(L / kEvalManyChunkMin, 1));
    *chunk = (L + want - 1) / want;
    return (uint32_t)((L + *chunk - 1) / *chunk);
}
static bool upoly_evalmany_direct(uint64_t L, uint64_t n, const EvalManyShape &sh) {
    static const uint64_t forced = env_u64("ZK_UPOLY_EVALMANY_DIRECT_MAX", kUpolyModel, 0, kEvalManyDirectCap);
    if (!sh.tree_ok) return true;
    if (forced != kUpolyModel) return sh.products <= forced;
    uint64_t chunk = 0;
    (void)upoly_evalmany_chunks(L, n, &chunk);
    const double direct_us = std::max(kEvalManyChainUs * (double)chunk, (double)sh.products / kEvalManyDirectRate);
    const double tree_us = kEvalManyTreeLog2Us * (double)sh.log_N * (double)sh.log_N + kEvalManyTreePerPoint * (double)(1ull << sh.log_N);
    return direct_us <= tree_us;
}
static int32_t upoly_evalmany_direct_run(zk_ctx *c, const uint64_t *p, uint64_t L, const uint64_t *xs, uint64_t n, uint64_t *out) {
    const uint64_t tiles = (n + kBlock - 1) / kBlock;
    if (tiles > 0x7fffffffull) return ZK_ERR_UNSUPPORTED;
    uint64_t chunk = 0;
    const uint32_t chunks = upoly_evalmany_chunks(L, n, &chunk);
    PoolScope ps(c);
    uint64_t *partials = out;
    if (chunks > 1) ZKCHK(ps.get(upoly_block_bytes((uint64_t)chunks * n), &partials));
    k_evalmany_direct<<<dim3((uint32_t)tiles, chunks), kBlock, 0, c->stream>>>(p, L, xs, n, chunk, c->fi->P, partials);
    if (chunks > 1) k_evalmany_sum<<<grid_for(n), kBlock, 0, c->stream>>>(partials, n, chunks, c->fi->P, out);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// Timing split for tools/upoly_evalmany_bench.py (zk_bench_upoly_evaluate_many), mk: marks after the up-sweep (0), the series inversion
// (1), the root vector (2) and the NTT levels of the down-sweep (3).
// out[i] = p(xs[i]), i < n, by the transposed subproduct tree over N = 2^log_N >= max(n, L) points (upoly_kernels.cuh).  Asynchronous.
// Device memory: the retained levels, (log_N - 7) N 32 bytes (416 MiB at 2^20, 8.5 GiB at 2^24), and 20 N-element blocks around them.
static int32_t upoly_evalmany_tree(zk_ctx *c, const uint64_t *p, uint64_t L, const uint64_t *xs, uint64_t n, uint32_t log_N, uint64_t *out,
                                   const PhaseEvents *mk) {
    const FieldParams &P = c->fi->P;
    const uint64_t N = 1ull << log_N;
    const size_t nb_bytes = (size_t)32 << log_N;
    const uint32_t bot = std::min<uint32_t>(log_N, kEvalManyBottomLog), n_lev = log_N - bot;   // kept: the levels bot .. log_N - 1
    const NttFuseArgs none = {0};
    PoolScope ps(c);
    uint64_t *xp = nullptr, *lev = nullptr, *mroot = nullptr, *T[3] = {nullptr, nullptr, nullptr}, *S = nullptr;
    ZKCHK(ps.get(nb_bytes, &xp));
    ZKCHK(ps.get(nb_bytes, &mroot));
    if (n_lev) {
        ZKCHK(ps.get(nb_bytes * n_lev, &lev));
        for (int q = 0; q < 3; ++q) ZKCHK(ps.get(nb_bytes, &T[q]));
        ZKCHK(ps.get(nb_bytes, &S));
    }
    auto level = [&](uint32_t l) { return l == log_N ? mroot : lev + 4 * ((uint64_t)(l - bot) << log_N); };
    // 1, 2. the points padded with zeros, and the up-sweep, m only: the direct levels, then two forward transforms and one inverse a level
    k_evalmany_pad<<<grid_for(N), kBlock, 0, c->stream>>>(xs, n, N, xp);
    k_interp_tree_direct<kEvalManyBottomLog, true><<<(uint32_t)((N + (1ull << kEvalManyBottomLog) - 1) >> kEvalManyBottomLog),
                                                     1 << kEvalManyBottomLog, 0, c->stream>>>(nullptr, xp, N, P, level(bot), nullptr);
    HIPCHK(hipGetLastError());
    for (uint32_t l = bot; l < log_N; ++l) {
        const uint64_t nb = N >> (l + 1), s = 1ull << l;
        const NttPlan *fw = nullptr, *iv = nullptr;
        ZKCHK(ntt_cached_plan(c, l + 1, false, &fw));
        ZKCHK(ntt_cached_plan(c, l + 1, true, &iv));
        const uint64_t *mc = level(l);
        const NttFuseArgs left = {s, 2 * s, 0, nullptr, nullptr}, right = {s, 2 * s, s, nullptr, nullptr};
        ZKCHK(ntt_run_batched(c, *fw, nb, mc, T[0], S, false, kNttBatchPad, left, kNttBatch, none));
        ZKCHK(ntt_run_batched(c, *fw, nb, mc, T[1], S, false, kNttBatchPad, right, kNttBatchMulAux, NttFuseArgs{0, 0, 0, T[0], nullptr}));
        ZKCHK(ntt_run_batched(c, *iv, nb, T[0], level(l + 1), S, true, kNttBatch, none, kNttBatchShift,
                              NttFuseArgs{0, 0, 0, const_cast<uint64_t *>(mc), nullptr}));
    }
    if (mk) ZKCHK(mk->mark(0));
    // 3. alpha = 1 / rev(M) mod z^N (upoly_inverse_series_into; R_0 = 1, so nothing is inverted)
    uint64_t *R = nullptr, *alpha = nullptr, *e = nullptr, *g = nullptr;
    ZKCHK(ps.get(nb_bytes, &R));
    ZKCHK(ps.get(nb_bytes, &alpha));
    k_evalmany_series<<<grid_for(N), kBlock, 0, c->stream>>>(level(log_N), N, P, R);
    HIPCHK(hipGetLastError());
    ZKCHK(upoly_inverse_series_into(c, R, N, N, alpha, nullptr));
    ZKCHK(ps.get(2 * nb_bytes, &e));
    ZKCHK(ps.get(nb_bytes, &g));
    if (mk) ZKCHK(mk->mark(1));
    // 4. b = the reversal of the first N coefficients of rev(c) alpha  (g and e are free again)
    uint64_t *bv[2] = {nullptr, nullptr};
    ZKCHK(ps.get(nb_bytes, &bv[0]));
    if (n_lev) ZKCHK(ps.get(nb_bytes, &bv[1]));
    k_evalmany_reverse<<<grid_for(N), kBlock, 0, c->stream>>>(p, L, N, g);
    HIPCHK(hipGetLastError());
    if (N > 1) {
        uint32_t lg = 0;
        ZKCHK(upoly_product_log(c, N, N, &lg));
        ZKCHK(upoly_mul_into(c, g, N, alpha, N, e, lg));
        k_evalmany_reverse<<<grid_for(N), kBlock, 0, c->stream>>>(e, N, N, bv[0]);
    } else {
        k_evalmany_pad<<<1, kBlock, 0, c->stream>>>(g, 1, 1, bv[0]);   // alpha = 1: b_0 = c_0
    }
    HIPCHK(hipGetLastError());
    if (mk) ZKCHK(mk->mark(2));
    // 5. down-sweep: the children's transforms again (pad on load), b's multiplied into both, two inverses keeping the upper halves
    uint32_t bc = 0;
    for (uint32_t l = log_N; l-- > bot; bc ^= 1) {
        const uint64_t nb = N >> (l + 1), s = 1ull << l;
        const NttPlan *fw = nullptr, *iv = nullptr;
        ZKCHK(ntt_cached_plan(c, l + 1, false, &fw));
        ZKCHK(ntt_cached_plan(c, l + 1, true, &iv));
        const uint64_t *mc = level(l);
        const NttFuseArgs left = {s, 2 * s, 0, nullptr, nullptr}, right = {s, 2 * s, s, nullptr, nullptr};
        ZKCHK(ntt_run_batched(c, *fw, nb, mc, T[1], S, false, kNttBatchPad, left, kNttBatch, none));
        ZKCHK(ntt_run_batched(c, *fw, nb, mc, T[2], S, false, kNttBatchPad, right, kNttBatch, none));
        ZKCHK(ntt_run_batched(c, *fw, nb, bv[bc], T[0], S, false, kNttBatch, none, kNttBatchMulAux, NttFuseArgs{0, 0, 0, T[1], T[2]}));
        ZKCHK(ntt_run_batched(c, *iv, nb, T[2], bv[bc ^ 1], S, true, kNttBatch, none, kNttBatchUpperAdd, NttFuseArgs{0, 0, 0, bv[bc], nullptr}));
        ZKCHK(ntt_run_batched(c, *iv, nb, T[1], bv[bc ^ 1], S, true, kNttBatch, none, kNttBatchUpperAdd, NttFuseArgs{0, 0, s, bv[bc], nullptr}));
    }
    if (mk) ZKCHK(mk->mark(3));
    // 6. the bottom: one workgroup per node of 2^bot points (only the nodes that hold real points)
    const uint64_t nodes = (n + (1ull << bot) - 1) >> bot;
    if (nodes > 0x7fffffffull) return ZK_ERR_UNSUPPORTED;
    k_evalmany_bottom<<<(uint32_t)nodes, 1 << kEvalManyBottomLog, 0, c->stream>>>(bv[bc], level(bot), xs, 1u << bot, n, P, out);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// out (n elements) = p (L coefficients) at the n points; path 0: the model / the switch, 1: direct, 2: tree
static int32_t upoly_evalmany_into(zk_ctx *c, const uint64_t *p, uint64_t L, const uint64_t *xs, uint64_t n, const EvalManyShape &sh,
                                   uint64_t *out, int32_t path, const PhaseEvents *mk) {
    if (!n) return ZK_OK;
    if (!L) {   // the empty fold: F::zero() at every point
        HIPCHK(hipMemsetAsync(out, 0, (size_t)n * 32, c->stream));
        return ZK_OK;
    }
    const bool direct = path == 1 || (path == 0 && upoly_evalmany_direct(L, n, sh));
    if (direct) return upoly_evalmany_direct_run(c, p, L, xs, n, out);
    if (!sh.tree_ok) return ZK_ERR_UNSUPPORTED;
    return upoly_evalmany_tree(c, p, L, xs, n, sh.log_N, out, mk);
}
// interpolate: weights by the closed form (one backward scan of 1, 1, 2, .., n-1 and one inversion), then the tree
static int32_t upoly_interpolate_into(zk_ctx *c, const uint64_t *ys, uint64_t n, uint64_t *out, const PhaseEvents *mk) {
    PoolScope ps(c);
    uint64_t *suf = nullptr, *inv = nullptr, *W = nullptr;
    ZKCHK(ps.get(upoly_block_bytes(n), &suf));
    ZKCHK(ps.get(upoly_block_bytes(1), &inv));
    ZKCHK(ps.get(upoly_block_bytes(n), &W));
    const uint64_t *tot = nullptr;
    ZKCHK(upoly_scan_prod(c, ps, nullptr, n, 1, suf, &tot));
    k_fe_invert_one<<<1, 64, 0, c->stream>>>(tot, inv, c->fi->P);
    k_interp_weights_index<<<grid_for(n), kBlock, 0, c->stream>>>(ys, suf, inv, n, c->fi->P, W);
    HIPCHK(hipGetLastError());
    if (mk) ZKCHK(mk->mark(0));
    return upoly_interp_tree(c, ps, W, nullptr, n, out, mk);
}
// interpolate_xy's weights d_i = prod_{j != i} (x_i - x_j): from ZK_UPOLY_INTERP_XY_TREE_MIN points on (and where the tree path of the
// multipoint evaluation is available) as M'(x_i), O(nx log^2 nx); below it by k_interp_denoms, O(nx m).  The same bits either way.
// The default is the smallest measured power of two from which the tree path is faster (profiles/upoly_evalmany.log, BN254, the two
// paths in alternating child processes: 2^12 6.0 ms against the kernel's 4.8, 2^14 8.1 against 13.9, 2^16 11.7 against 50.0; the two
// passes of every figure agree within 0.5 %).
static constexpr uint64_t kInterpXyTreeMinDefault = 1ull << 14;
static uint64_t upoly_interp_xy_tree_min() {
    static const uint64_t v = env_u64("ZK_UPOLY_INTERP_XY_TREE_MIN", kInterpXyTreeMinDefault, 1, 1ull << 40);
    return v;
}
// interpolate_xy over nx points with m = min(nx, ny) weights; *bad_flag (device word, zeroed here) = 1 on a repeated x at an index < m
static int32_t upoly_interpolate_xy_into(zk_ctx *c, const uint64_t *xs, uint64_t nx, const uint64_t *ys, uint64_t m, uint64_t *out,
                                         uint32_t *bad_flag, const PhaseEvents *mk) {
    PoolScope ps(c);
    uint64_t *d = nullptr, *pre = nullptr, *suf = nullptr, *inv = nullptr;
    ZKCHK(ps.get(upoly_block_bytes(nx), &d));
    ZKCHK(ps.get(upoly_block_bytes(nx), &pre));
    ZKCHK(ps.get(upoly_block_bytes(nx), &suf));
    ZKCHK(ps.get(upoly_block_bytes(1), &inv));
    HIPCHK(hipMemsetAsync(bad_flag, 0, 4, c->stream));
    EvalManyShape sh;
    if (nx >= upoly_interp_xy_tree_min() && upoly_evalmany_shape(c, nx, nx, &sh) == ZK_OK && sh.tree_ok) {
        // d_i = M'(x_i): M' is the tree's P for unit weights (P = sum_i M / (x - x_i)), evaluated at all the points by the tree path
        PoolScope inner(c);
        uint64_t *ones = nullptr, *dM = nullptr;
        ZKCHK(inner.get(upoly_block_bytes(nx), &ones));
        ZKCHK(inner.get(upoly_block_bytes(nx), &dM));
        k_fe_fill_one<<<grid_for(nx), kBlock, 0, c->stream>>>(ones, nx, c->fi->P);
        HIPCHK(hipGetLastError());
        ZKCHK(upoly_interp_tree(c, inner, ones, xs, nx, dM, nullptr));
        ZKCHK(upoly_evalmany_tree(c, dM, nx, xs, nx, sh.log_N, d, nullptr));
        k_interp_denoms_fix<<<grid_for(nx), kBlock, 0, c->stream>>>(d, nx, m, c->fi->P, bad_flag);
    } else {
        k_interp_denoms<<<(uint32_t)((nx + kBlock - 1) / kBlock), kBlock, 0, c->stream>>>(xs, nx, m, c->fi->P, d, bad_flag);
    }
    HIPCHK(hipGetLastError());
    const uint64_t *tot = nullptr, *tot2 = nullptr;
    ZKCHK(upoly_scan_prod(c, ps, d, nx, 0, pre, &tot));
    ZKCHK(upoly_scan_prod(c, ps, d, nx, 1, suf, &tot2));
    k_fe_invert_one<<<1, 64, 0, c->stream>>>(tot, inv, c->fi->P);
    k_interp_weights_xy<<<grid_for(nx), kBlock, 0, c->stream>>>(ys, pre, suf, inv, nx, m, c->fi->P, d);   // w over d
    HIPCHK(hipGetLastError());
    if (mk) ZKCHK(mk->mark(0));
    return upoly_interp_tree(c, ps, d, xs, nx, out, mk);
}
extern "C" int32_t zk_upoly_interpolate(zk_ctx *c, const zk_upoly *ys, zk_upoly **out) {
    if (!c || !ys || !out) return ZK_ERR_BAD_ARG;
    if (ys->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    uint32_t lg = 0;
    ZKCHK(upoly_interp_log(c, ys->len, &lg));
    ZKCHK(use_device(c));
    UpolyHolder o;
    ZKCHK(upoly_alloc(c, ys->len, o.put()));   // n = 0: the empty polynomial
    if (ys->len) ZKCHK(upoly_interpolate_into(c, ys->d, ys->len, o->d, nullptr));
    *out = o.release();
    return ZK_OK;
}
// the one host wait: the repeated-x flag
static int32_t upoly_read_flag(zk_ctx *c, const uint32_t *flag, bool *set) {
    HIPCHK(hipMemcpyAsync(c->h_pinned, flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *set = *reinterpret_cast<volatile uint32_t *>(c->h_pinned) != 0;
    return ZK_OK;
}
extern "C" int32_t zk_upoly_interpolate_xy(zk_ctx *c, const zk_upoly *xs, const zk_upoly *ys, zk_upoly **out) {
    if (!c || !xs || !ys || !out) return ZK_ERR_BAD_ARG;
    if (xs->ctx != c || ys->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    const uint64_t nx = xs->len, m = std::min(xs->len, ys->len);
    uint32_t lg = 0;
    ZKCHK(upoly_interp_log(c, nx, &lg));
    ZKCHK(use_device(c));
    UpolyHolder o;
    ZKCHK(upoly_alloc(c, m ? nx : 0, o.put()));   // no weight: the empty polynomial (the zip of :59 is empty)
    if (!m) {
        *out = o.release();
        return ZK_OK;
    }
    PoolBlock flag;
    ZKCHK(flag.alloc(c, 32));
    ZKCHK(upoly_interpolate_xy_into(c, xs->d, nx, ys->d, m, o->d, flag.as<uint32_t>(), nullptr));
    bool bad = false;
    ZKCHK(upoly_read_flag(c, flag.as<uint32_t>(), &bad));
    if (bad) return ZK_ERR_PANIC_INVERSE;
    *out = o.release();
    return ZK_OK;
}
extern "C" int32_t zk_upoly_interpolate_host(zk_ctx *c, const uint64_t *ys, uint64_t n, uint64_t *out) {
    if (!c || (n && (!ys || !out))) return ZK_ERR_BAD_ARG;
    if (!n) return ZK_OK;
    uint32_t lg = 0;
    ZKCHK(upoly_interp_log(c, n, &lg));   // before anything is read or allocated
    UpolyHolder py, po;
    ZKCHK(zk_upoly_upload(c, ys, n, py.put()));
    ZKCHK(zk_upoly_interpolate(c, py.get(), po.put()));
    return zk_upoly_download(c, po.get(), out);
}
extern "C" int32_t zk_upoly_interpolate_xy_host(zk_ctx *c, const uint64_t *xs, uint64_t nx, const uint64_t *ys, uint64_t ny, uint64_t *out) {
    if (!c || (nx && !xs) || (ny && !ys)) return ZK_ERR_BAD_ARG;
    if (!nx || !ny) return ZK_OK;   // empty result: nothing is written
    if (!out) return ZK_ERR_BAD_ARG;
    uint32_t lg = 0;
    ZKCHK(upoly_interp_log(c, nx, &lg));
    UpolyHolder px, py, po;
    ZKCHK(zk_upoly_upload(c, xs, nx, px.put()));
    ZKCHK(zk_upoly_upload(c, ys, std::min(nx, ny), py.put()));
    ZKCHK(zk_upoly_interpolate_xy(c, px.get(), py.get(), po.put()));
    return zk_upoly_download(c, po.get(), out);
}

// evaluate_many: out[i] = p.evaluate(xs[i]) (univariate_poly.rs:29-40) for a vector of points.  Asynchronous, no host wait.
extern "C" int32_t zk_upoly_evaluate_many(zk_ctx *c, const zk_upoly *p, const zk_upoly *xs, zk_upoly **out) {
    if (!c || !p || !xs || !out) return ZK_ERR_BAD_ARG;
    if (p->ctx != c || xs->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    EvalManyShape sh;
    ZKCHK(upoly_evalmany_shape(c, p->len, xs->len, &sh));
    ZKCHK(use_device(c));
    UpolyHolder o;
    ZKCHK(upoly_alloc(c, xs->len, o.put()));   // n = 0: the empty handle
    ZKCHK(upoly_evalmany_into(c, p->d, p->len, xs->d, xs->len, sh, o->d, 0, nullptr));
    *out = o.release();
    return ZK_OK;
}
extern "C" int32_t zk_upoly_evaluate_many_host(zk_ctx *c, const uint64_t *coeffs, uint64_t len, const uint64_t *xs, uint64_t n, uint64_t *out) {
    if (!c || (!coeffs && len) || (!xs && n)) return ZK_ERR_BAD_ARG;
    if (!n) return ZK_OK;   // empty result: nothing is written
    EvalManyShape sh;
    ZKCHK(upoly_evalmany_shape(c, len, n, &sh));   // before anything is read or allocated
    if (!out) return ZK_ERR_BAD_ARG;
    UpolyHolder pp, px, po;
    ZKCHK(zk_upoly_upload(c, coeffs, len, pp.put()));
    ZKCHK(zk_upoly_upload(c, xs, n, px.put()));
    ZKCHK(zk_upoly_evaluate_many(c, pp.get(), px.get(), po.put()));
    return zk_upoly_download(c, po.get(), out);
}


// ---- division with remainder and the series inverse as calls -------------------------------------------
// The reference has no division: tests/divrem_ref.py is the definition.  Lengths fix every shape (degree() = len - 1, nothing trimmed).
// Three paths with the same bytes (the result is unique): the one-workgroup schoolbook kernel up to ZK_UPOLY_DIVREM_DIRECT_MAX
// coefficients of a (at most kDivremDirectMax; 0: never), the affine scan for lb = 2 above it (ZK_UPOLY_DIVREM_LINEAR = 0: never), and
// Newton: q = rev_k((rev(a) mod z^k) (1 / rev(b) mod z^k) mod z^k), r = a - (q mod z^m)(b mod z^m) mod z^m for m = lb - 1.
// The default keeps the direct kernel below the smallest measured size at which Newton wins (profiles/upoly_divrem.log, MI355X, BN254,
// la = 2 lb: 2^9 1.25 ms against 1.27, 2^10 2.22 against 1.54, 2^11 5.1 against 1.8; nothing between 2^9 and 2^10 was measured).
static constexpr uint64_t kDivremDirectDefault = 1023;
enum DivremPath { kDivNone = 0, kDivDirect = 1, kDivLinear = 2, kDivNewton = 3 };   // kDivNone: la < lb, q empty and r = a
struct DivremShape {
    int path;
    uint64_t k;   // len(q)
};
// The length rule of zk_upoly_divrem, checked before anything is read or allocated.  forced: 0 = the switches, 1 .. 3 = that path
// (the measurement hook; ZK_ERR_BAD_ARG where it is not available).
static int32_t upoly_divrem_shape(const zk_ctx *c, uint64_t la, uint64_t lb, int32_t forced, DivremShape *sh) {
    static const uint64_t direct_max = std::min<uint64_t>(env_u64("ZK_UPOLY_DIVREM_DIRECT_MAX", kDivremDirectDefault, 0, 1ull << 40), kDivremDirectMax);
    static const bool linear_on = env_u64("ZK_UPOLY_DIVREM_LINEAR", 1, 0, 1) != 0;
    if (la > (1ull << kMaxVars) || lb > (1ull << kMaxVars)) return ZK_ERR_UNSUPPORTED;
    sh->path = kDivNone;
    sh->k = 0;
    if (la < lb) return forced ? ZK_ERR_BAD_ARG : ZK_OK;
    const uint64_t k = la - lb + 1, m = lb - 1;
    sh->k = k;
    uint32_t lg = 0;
    const bool newton_ok = upoly_series_log(c, k, &lg) == ZK_OK && (!m || upoly_product_log(c, std::min(m, k), m, &lg) == ZK_OK);
    if (forced) {
        const bool ok = forced == kDivDirect ? la <= kDivremDirectMax : forced == kDivLinear ? lb == 2 : newton_ok;
        if (!ok) return ZK_ERR_BAD_ARG;
        sh->path = forced;
        return ZK_OK;
    }
    if (lb == 2 && la > direct_max && linear_on) sh->path = kDivLinear;
    else if (la <= direct_max) sh->path = kDivDirect;
    else if (newton_ok) sh->path = kDivNewton;
    else return ZK_ERR_UNSUPPORTED;
    return ZK_OK;
}
static int32_t upoly_divrem_direct_run(zk_ctx *c, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, uint64_t *q, uint64_t *r,
                                       uint32_t *flag) {
    const size_t lds = (size_t)la * 32;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_upoly_divrem_direct), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_upoly_divrem_direct<<<1, kBlock, lds, c->stream>>>(a, (uint32_t)la, b, (uint32_t)lb, c->fi->P, q, r, flag);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
static int32_t upoly_divrem_linear_run(zk_ctx *c, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t *q, uint64_t *r, uint32_t *flag) {
    const uint64_t nc = (la + kScanChunk - 1) / kScanChunk;   // la <= 2^40: at most 2^28 chunks
    PoolScope ps(c);
    uint64_t *consts = nullptr, *tot = nullptr;
    ZKCHK(ps.get(upoly_block_bytes(4), &consts));
    ZKCHK(ps.get(upoly_block_bytes(nc + 1), &tot));
    k_divlin_setup<<<1, 64, 0, c->stream>>>(b, c->fi->P, consts, flag);
    k_divlin_partial<<<(uint32_t)nc, kBlock, 0, c->stream>>>(a, la, consts, c->fi->P, tot);
    k_divlin_carry<<<1, kBlock, 0, c->stream>>>(tot, (uint32_t)nc, consts, c->fi->P);
    if (q) k_divlin_apply<<<(uint32_t)nc, kBlock, 0, c->stream>>>(a, la, consts, tot, c->fi->P, q);
    HIPCHK(hipGetLastError());
    if (r) HIPCHK(hipMemcpyAsync(r, tot + 4 * nc, 32, hipMemcpyDeviceToDevice, c->stream));   // r[0] = S[0] = a(z)
    return ZK_OK;
}
// Timing split for tools/upoly_divrem_bench.py (zk_bench_upoly_divrem), mk: marks after the series inverse (0) and the quotient product (1).
static int32_t upoly_divrem_newton_run(zk_ctx *c, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, uint64_t *q, uint64_t *r,
                                       uint32_t *flag, const PhaseEvents *mk) {
    const FieldParams &P = c->fi->P;
    const uint64_t k = la - lb + 1, m = lb - 1, lbk = std::min(lb, k);
    PoolScope ps(c);
    uint64_t *ra = nullptr, *rb = nullptr, *alpha = nullptr, *prod = nullptr;
    ZKCHK(ps.get(upoly_block_bytes(k), &ra));
    ZKCHK(ps.get(upoly_block_bytes(lbk), &rb));
    ZKCHK(ps.get(upoly_block_bytes(k), &alpha));
    ZKCHK(ps.get(upoly_block_bytes(2 * k), &prod));
    if (!q) ZKCHK(ps.get(upoly_block_bytes(k), &q));   // the remainder needs the quotient
    k_upoly_reverse_top<<<grid_for(k), kBlock, 0, c->stream>>>(a, la, k, ra);
    k_upoly_reverse_top<<<grid_for(lbk), kBlock, 0, c->stream>>>(b, lb, lbk, rb);
    HIPCHK(hipGetLastError());
    ZKCHK(upoly_inverse_series_into(c, rb, lbk, k, alpha, flag));
    if (mk) ZKCHK(mk->mark(0));
    uint32_t lg = 0;
    ZKCHK(upoly_product_log(c, k, k, &lg));
    ZKCHK(upoly_mul_into(c, ra, k, alpha, k, prod, lg));
    k_evalmany_reverse<<<grid_for(k), kBlock, 0, c->stream>>>(prod, k, k, q);   // q[j] = prod[k - 1 - j]
    HIPCHK(hipGetLastError());
    if (mk) ZKCHK(mk->mark(1));
    if (!r || !m) return ZK_OK;
    // only the low m coefficients of q b: the prefixes' product (never the la-long one), then one subtraction
    const uint64_t qm = std::min(m, k);
    uint64_t *qb = nullptr;
    ZKCHK(ps.get(upoly_block_bytes(qm + m), &qb));
    ZKCHK(upoly_product_log(c, qm, m, &lg));
    ZKCHK(upoly_mul_into(c, q, qm, b, m, qb, lg));
    k_upoly_sub_trunc<<<grid_for(m), kBlock, 0, c->stream>>>(a, qb, m, P, r);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// q (k elements) and r (lb - 1 elements), either of them null, for la >= lb; *flag (a zeroed device word) |= 1 on b[lb - 1] = 0
static int32_t upoly_divrem_into(zk_ctx *c, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, const DivremShape &sh, uint64_t *q,
                                 uint64_t *r, uint32_t *flag, const PhaseEvents *mk) {
    if (lb == 1) r = nullptr;   // the empty remainder
    switch (sh.path) {
        case kDivDirect: return upoly_divrem_direct_run(c, a, la, b, lb, q, r, flag);
        case kDivLinear: return upoly_divrem_linear_run(c, a, la, b, q, r, flag);
        case kDivNewton: return upoly_divrem_newton_run(c, a, la, b, lb, q, r, flag, mk);
        default: return ZK_ERR_BAD_ARG;
    }
}
extern "C" int32_t zk_upoly_divrem(zk_ctx *c, const zk_upoly *a, const zk_upoly *b, zk_upoly **out_q, zk_upoly **out_r) {
    if (!c || !a || !b || (!out_q && !out_r)) return ZK_ERR_BAD_ARG;
    if (a->ctx != c || b->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (b->len == 0) return ZK_ERR_BAD_ARG;
    DivremShape sh;
    ZKCHK(upoly_divrem_shape(c, a->len, b->len, 0, &sh));
    ZKCHK(use_device(c));
    UpolyHolder q, r;
    if (sh.path == kDivNone) {   // la < lb: q empty, r a copy of a
        if (out_q) ZKCHK(upoly_alloc(c, 0, q.put()));
        if (out_r) {
            ZKCHK(upoly_alloc(c, a->len, r.put()));
            if (a->len) HIPCHK(hipMemcpyAsync(r->d, a->d, (size_t)a->len * 32, hipMemcpyDeviceToDevice, c->stream));
        }
    } else {
        if (out_q) ZKCHK(upoly_alloc(c, sh.k, q.put()));
        if (out_r) ZKCHK(upoly_alloc(c, b->len - 1, r.put()));
        PoolBlock flag;
        ZKCHK(flag.alloc(c, 32));
        HIPCHK(hipMemsetAsync(flag.as<uint32_t>(), 0, 4, c->stream));
        ZKCHK(upoly_divrem_into(c, a->d, a->len, b->d, b->len, sh, out_q ? q->d : nullptr, out_r ? r->d : nullptr, flag.as<uint32_t>(), nullptr));
        bool bad = false;
        ZKCHK(upoly_read_flag(c, flag.as<uint32_t>(), &bad));
        if (bad) return ZK_ERR_PANIC_INVERSE;
    }
    if (out_q) *out_q = q.release();
    if (out_r) *out_r = r.release();
    return ZK_OK;
}
extern "C" int32_t zk_upoly_inverse_series(zk_ctx *c, const zk_upoly *f, uint64_t k, zk_upoly **out) {
    if (!c || !f || !out) return ZK_ERR_BAD_ARG;
    if (f->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    uint32_t lg = 0;
    if (k) ZKCHK(upoly_series_log(c, k, &lg));
    ZKCHK(use_device(c));
    if (!k) return upoly_alloc(c, 0, out);
    if (!f->len) return ZK_ERR_PANIC_INVERSE;   // f = 0: nothing to invert, no wait
    UpolyHolder o;
    ZKCHK(upoly_alloc(c, k, o.put()));
    PoolBlock flag;
    ZKCHK(flag.alloc(c, 32));
    HIPCHK(hipMemsetAsync(flag.as<uint32_t>(), 0, 4, c->stream));
    ZKCHK(upoly_inverse_series_into(c, f->d, f->len, k, o->d, flag.as<uint32_t>()));
    bool bad = false;
    ZKCHK(upoly_read_flag(c, flag.as<uint32_t>(), &bad));
    if (bad) return ZK_ERR_PANIC_INVERSE;
    *out = o.release();
    return ZK_OK;
}
extern "C" int32_t zk_upoly_divrem_host(zk_ctx *c, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, uint64_t *out_q,
                                        uint64_t *out_r) {
    if (!c || (!a && la) || !b || !lb) return ZK_ERR_BAD_ARG;
    DivremShape sh;
    ZKCHK(upoly_divrem_shape(c, la, lb, 0, &sh));   // before anything is read or allocated
    const uint64_t lr = sh.path == kDivNone ? la : lb - 1;
    if ((sh.k && !out_q) || (lr && !out_r)) return ZK_ERR_BAD_ARG;
    UpolyHolder pa, pb, pq, pr;
    ZKCHK(zk_upoly_upload(c, a, la, pa.put()));
    ZKCHK(zk_upoly_upload(c, b, lb, pb.put()));
    ZKCHK(zk_upoly_divrem(c, pa.get(), pb.get(), pq.put(), pr.put()));
    ZKCHK(zk_upoly_download(c, pq.get(), out_q));
    return zk_upoly_download(c, pr.get(), out_r);
}
extern "C" int32_t zk_upoly_inverse_series_host(zk_ctx *c, const uint64_t *f, uint64_t lf, uint64_t k, uint64_t *out) {
    if (!c || (!f && lf)) return ZK_ERR_BAD_ARG;
    if (!k) return ZK_OK;   // empty result: nothing is written
    uint32_t lg = 0;
    ZKCHK(upoly_series_log(c, k, &lg));   // before anything is read or allocated
    if (!out) return ZK_ERR_BAD_ARG;
    if (!lf) return ZK_ERR_PANIC_INVERSE;
    UpolyHolder pf, po;
    ZKCHK(zk_upoly_upload(c, f, std::min(lf, k), pf.put()));   // coefficients from z^k on do not enter
    ZKCHK(zk_upoly_inverse_series(c, pf.get(), k, po.put()));
    return zk_upoly_download(c, po.get(), out);
}

// ------------------------------------------------------------------------------------------------------------
// measurement hooks
// ------------------------------------------------------------------------------------------------------------
// interpolate (xs null) or interpolate_xy of n points, `reps` times; out_ms[0..5) = average ms of the whole call and of its weights,
// direct levels, NTT levels and block merges (HIP events on the context's stream; the call's pool blocks are warm after the first rep)
extern "C" int32_t zk_bench_upoly_interp(zk_ctx *c, const zk_upoly *xs, const zk_upoly *ys, int32_t reps, double *out_ms) {
    if (!c || !ys || !out_ms || reps < 1) return ZK_ERR_BAD_ARG;
    if (ys->ctx != c || (xs && xs->ctx != c)) return ZK_ERR_CONTEXT_MISMATCH;
    const uint64_t n = xs ? xs->len : ys->len;
    if (!n || (xs && ys->len < n)) return ZK_ERR_BAD_ARG;
    uint32_t lg = 0;
    ZKCHK(upoly_interp_log(c, n, &lg));
    ZKCHK(use_device(c));
    PoolBlock o_block, flag_block;
    ZKCHK(o_block.alloc(c, upoly_block_bytes(n)));
    ZKCHK(flag_block.alloc(c, 32));
    uint64_t *o = o_block.as();
    uint32_t *flag = flag_block.as<uint32_t>();
    PhaseEvents mk(c);
    ZKCHK(mk.create(3));
    return mk.run(c, 0, reps, true, [&] {
        return xs ? upoly_interpolate_xy_into(c, xs->d, n, ys->d, n, o, flag, &mk) : upoly_interpolate_into(c, ys->d, n, o, &mk);
    }, out_ms);
}
// zk_upoly_evaluate_many of p at xs, `reps` times after one untimed run, on path 0 (the model / the switch), 1 (direct) or 2 (tree);
// out_ms[0..6) = average ms of the whole call and, on the tree path, of its up-sweep, series inversion, root vector, NTT levels of the
// down-sweep and bottom kernel (zeros on the direct path)
extern "C" int32_t zk_bench_upoly_evaluate_many(zk_ctx *c, const zk_upoly *p, const zk_upoly *xs, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !p || !xs || !out_ms || reps < 1 || path < 0 || path > 2) return ZK_ERR_BAD_ARG;
    if (p->ctx != c || xs->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (!p->len || !xs->len) return ZK_ERR_BAD_ARG;
    EvalManyShape sh;
    ZKCHK(upoly_evalmany_shape(c, p->len, xs->len, &sh));
    if (path == 2 && !sh.tree_ok) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    const bool tree = path == 2 || (path == 0 && !upoly_evalmany_direct(p->len, xs->len, sh));
    PoolBlock o_block;
    ZKCHK(o_block.alloc(c, upoly_block_bytes(xs->len)));
    PhaseEvents mk(c);
    ZKCHK(mk.create(4));
    // one warm-up run: plans, twiddle tables, pool blocks
    return mk.run(c, 1, reps, tree, [&] {
        return upoly_evalmany_into(c, p->d, p->len, xs->d, xs->len, sh, o_block.as(), tree ? 2 : 1, &mk);
    }, out_ms);
}
// zk_upoly_divrem of a by b (la >= lb >= 1, b's leading coefficient not zero), both results, `reps` times after one untimed run, on
// path 0 (the switches), 1 (direct), 2 (linear) or 3 (Newton); ZK_ERR_BAD_ARG where the path is not available.  out_ms[0..4) = average
// ms of the whole call and, on the Newton path, of its series inverse, quotient product and remainder (zeros on the other paths)
extern "C" int32_t zk_bench_upoly_divrem(zk_ctx *c, const zk_upoly *a, const zk_upoly *b, int32_t path, int32_t reps, double *out_ms) {
    if (!c || !a || !b || !out_ms || reps < 1 || path < 0 || path > 3) return ZK_ERR_BAD_ARG;
    if (a->ctx != c || b->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (!b->len || a->len < b->len) return ZK_ERR_BAD_ARG;
    DivremShape sh;
    ZKCHK(upoly_divrem_shape(c, a->len, b->len, path, &sh));
    ZKCHK(use_device(c));
    const bool newton = sh.path == kDivNewton;
    PoolBlock q_block, r_block, flag_block;
    ZKCHK(q_block.alloc(c, upoly_block_bytes(sh.k)));
    ZKCHK(r_block.alloc(c, upoly_block_bytes(b->len)));
    ZKCHK(flag_block.alloc(c, 32));
    HIPCHK(hipMemsetAsync(flag_block.as<uint32_t>(), 0, 4, c->stream));
    PhaseEvents mk(c);
    ZKCHK(mk.create(2));
    // one warm-up run: plans, twiddle tables, pool blocks
    return mk.run(c, 1, reps, newton, [&] {
        return upoly_divrem_into(c, a->d, a->len, b->d, b->len, sh, q_block.as(), r_block.as(), flag_block.as<uint32_t>(), &mk);
    }, out_ms);
}
extern "C" int32_t zk_bench_ntt(zk_ctx *c, const zk_mle *in, int32_t inverse, zk_mle *out, int32_t reps, double *out_ms) {
    if (!c || !in || !out || !out_ms || reps <= 0) return ZK_ERR_BAD_ARG;
    // builds the twiddle tables, then as many untimed transforms as timed ones: the passes are ALU-bound and follow the shader
    // clock, which keeps climbing for ~20 ms after idle (r02 kernel trace: 986 -> 720 us for the same kernel over 12 transforms)
    return timed_span(c, reps + 1, AfterWarm::kNoWait, reps, [&] { return zk_ntt(c, in, inverse, out); }, out_ms);
}
