// kernels.cuh -- gfx950 kernels for the MLE fold / evaluate / serialisation path (the sumcheck prover's own: sumcheck_kernels.cuh).
//
// Data layout in HBM: a table is a dense array of 2^m elements, 32 B each (8 x u32, Montgomery), index bit
// (m-1-v) <-> variable v, i.e. variable 0 is the index MSB (polynomial/src/multilinear/pairing_index.rs:61-65).
// The sumcheck fold always consumes variable 0, so a round touches the two contiguous half-streams
// [0, half) and [half, 2*half): every lane reads whole 32-B elements, a wave reads 2 KiB contiguous runs.
//
// All kernels are grid-stride with 256-thread workgroups (4 waves); grids are sized >> 256 CUs by the host.
// These are HBM-streaming integer kernels: no LDS tiling is needed for the fold itself (no reuse), LDS is used
// for the workgroup reductions of the evaluate kernels.  No MFMA (256-bit modular integer ops).
#pragma once
#include "common.cuh"

namespace zk {

// pairing_index.rs:16-20 insert_bit(val, index, 0)
ZK_D uint64_t insert_zero_bit(uint64_t val, uint32_t pos) {
    const uint64_t low = val & ((1ull << pos) - 1ull);
    return ((val >> pos) << (pos + 1)) | low;
}

// ---- MultiLinearPolynomial::partial_evaluate, one assignment (evaluation_form.rs:55-70) ----------------------
// out[j] = left - r*(left - right), (left,right) = index_pair(m, initial_var)[j], pos = m-1-initial_var.
// The reference's r==0 / r==1 shortcuts (:61-62) are the same values, so they are not special-cased.
// Out of place (in != out) for general pos; in place is race-free only for the MSB fold (pos = m-1).
__global__ __launch_bounds__(kBlock) void k_fold(const uint64_t *in, uint64_t *out,
                                                 uint64_t pairs, uint32_t pos, FieldParams P, Mul29 r) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < pairs; j += stride) {
        const uint64_t l = insert_zero_bit(j, pos);
        const Fe lo = fe_load(in, l);
        const Fe hi = fe_load(in, l | (1ull << pos));
        const Fe d = fe_sub(lo, hi, P);
        fe_store(out, j, fe_sub(lo, fe_mul29(d, r, P), P));   // r is prepared on the host: mul29_prepare(challenge)
    }
}

// ---- the sumcheck fold (variable 0 = index MSB) as the bandwidth kernel --------------------------------------------
// Same arithmetic as k_fold with pos = m-1, different data movement: a wave moves 64 consecutive elements of each of
// the three streams (lo, hi, out) as two fully coalesced 1-KiB dwordx4 accesses (lane l touches bytes [16l, 16l+16) of
// the run), and lanes 2i / 2i+1 swap halves with one DPP quad_perm so each lane ends up owning one whole element
// (even lane: element i, odd lane: element 32+i).  All accesses are nontemporal: the table is streamed once.
// Measured on MI355X (tools/mb/mb_stream.hip, 2^24): 5.8-5.9 TB/s vs 5.4 TB/s for the 32-B-per-lane form.
// half = 2^(m-1) >= 64 (a multiple of 64).  Out of place or in place (a wave reads its 64 lo/hi elements before
// writing the 64 outputs at the lo positions; no other wave touches them).
__global__ __launch_bounds__(kBlock) void k_fold_msb(const uint64_t *in, uint64_t *out, uint64_t half, FieldParams P, Mul29 r) {
    const uint32_t lane = threadIdx.x & 63;
    const bool odd = lane & 1;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint4 *in4 = reinterpret_cast<const uint4 *>(in);
    uint4 *out4 = reinterpret_cast<uint4 *>(out);
    for (uint64_t e0 = wave * 64; e0 < half; e0 += nwaves * 64) {
        const uint64_t c0 = 2 * e0 + lane;   // element e occupies uint4 slots 2e, 2e+1
        const uint4 la = nt_load16(in4 + c0), lb = nt_load16(in4 + c0 + 64);
        const uint4 ha = nt_load16(in4 + c0 + 2 * half), hb = nt_load16(in4 + c0 + 2 * half + 64);
        const Fe lo = pair_gather(la, lb, odd), hi = pair_gather(ha, hb, odd);
        const Fe o = fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P);
        uint4 oa, ob;
        pair_scatter(o, odd, oa, ob);
        nt_store16(oa, out4 + c0);
        nt_store16(ob, out4 + c0 + 64);
    }
}

// The same data movement for ANY fold position pos >= 6 (partial_evaluate with initial_var > 0, evaluation_form.rs:55-70): the pair
// partner of an element sits 2^pos >= 64 elements away, so 64 consecutive outputs still read two contiguous 64-element runs --
// block b = e / 2^pos of the output reads in[b * 2^(pos+1) + off] and in[b * 2^(pos+1) + 2^pos + off].  k_fold_msb is the case
// of one block.  Out of place only (a later block's inputs are an earlier block's output positions).  Measured (bench rows_2p24):
// the 32-byte-per-lane k_fold reaches 0.62-0.66 of the HBM peak at 2^24, this form the MSB fold's 0.79.
__global__ __launch_bounds__(kBlock) void k_fold_run(const uint64_t *in, uint64_t *out, uint64_t pairs, uint32_t pos, FieldParams P, Mul29 r) {
    const uint32_t lane = threadIdx.x & 63;
    const bool odd = lane & 1;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint4 *in4 = reinterpret_cast<const uint4 *>(in);
    uint4 *out4 = reinterpret_cast<uint4 *>(out);
    const uint64_t span = 1ull << pos;
    for (uint64_t e0 = wave * 64; e0 < pairs; e0 += nwaves * 64) {
        const uint64_t lo0 = ((e0 >> pos) << (pos + 1)) | (e0 & (span - 1));   // insert_zero_bit(e0, pos): first element of the lo run
        const uint64_t cl = 2 * lo0 + lane, co = 2 * e0 + lane;                // element e occupies uint4 slots 2e, 2e+1
        const uint4 la = nt_load16(in4 + cl), lb = nt_load16(in4 + cl + 64);
        const uint4 ha = nt_load16(in4 + cl + 2 * span), hb = nt_load16(in4 + cl + 2 * span + 64);
        const Fe lo = pair_gather(la, lb, odd), hi = pair_gather(ha, hb, odd);
        const Fe o = fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P);
        uint4 oa, ob;
        pair_scatter(o, odd, oa, ob);
        nt_store16(oa, out4 + co);
        nt_store16(ob, out4 + co + 64);
    }
}

// The same data movement for the LOW six fold positions (pos < 6: the pair partner is 1..32 elements away, inside the wave's
// run).  A wave reads 128 consecutive elements as two coalesced 64-element runs A and B (run_load: lane l owns element
// own(l) = (l >> 1) + 32 (l & 1) of each), so a lane holds one element of a pair of A and one of a pair of B; bit pos of own(l)
// says which side.  ONE exchange with the partner lane (own index differing in bit pos) hands the "low" lane the whole A pair
// and the "high" lane the whole B pair (the low lane sends its B element and receives the partner's A element, the high lane
// the other way round), every lane folds one pair, and a second lane permutation puts output own(l) of the wave's 64 outputs
// on lane l for the coalesced store.  Both permutations are ds_bpermute pulls (8 words each): a few LDS-crossbar cycles per
// 6 KiB of HBM traffic.  Out of place only; pairs a multiple of 64.  Until round 5 these positions ran on k_fold (32 bytes
// per lane: 0.63 of the HBM peak at 2^24 against 0.72-0.73 for the run forms).
ZK_D Fe lane_pull(const Fe &v, uint32_t src_lane) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), (int)v.v[i]);
    return r;
}
__global__ __launch_bounds__(kBlock) void k_fold_low(const uint64_t *in, uint64_t *out, uint64_t pairs, uint32_t pos, FieldParams P, Mul29 r) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint32_t own = pair_owned(lane);
    const bool high = (own >> pos) & 1u;
    const uint32_t partner_own = own ^ (1u << pos);
    const uint32_t partner = ((partner_own & 31u) << 1) | (partner_own >> 5);          // the lane that owns partner_own
    // this lane computes output q = 32 * high + (own without bit pos); the store wants output own(l) on lane l
    const uint32_t want = own, want_half = want >> 5, want_low = want & 31u;
    const uint32_t src_own = (((want_low >> pos) << (pos + 1)) | (want_low & ((1u << pos) - 1u))) | (want_half << pos);
    const uint32_t src = ((src_own & 31u) << 1) | (src_own >> 5);
    for (uint64_t e0 = wave * 64; e0 < pairs; e0 += nwaves * 64) {
        const Fe a = run_load_nt(in + 4 * (2 * e0), lane), b = run_load_nt(in + 4 * (2 * e0 + 64), lane);
        const Fe got = lane_pull(high ? a : b, partner);
        const Fe lo = high ? got : a, hi = high ? b : got;
        const Fe o = fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P);
        run_store_nt(out + 4 * e0, lane, lane_pull(o, src));
    }
}

// V consecutive MSB folds in one pass (evaluate, evaluation_form.rs:83-89: n folds in a row at KNOWN assignments): a thread
// reads the 2^V elements that share the low index j = idx mod 2^(m-V) (element c = (x0..x_{V-1}) sits at c * n_out + j),
// folds variable 0 over the pairs (c, c + 2^(V-1)), then variable 1, ... exactly in the reference's order, and writes one
// element: 1/V of the launches and (2^V + 1) / (3 * (2^V - 1)) of the traffic of V single folds.  In place is safe
// (index j is only touched by its own thread).
struct FoldChallenges {
    Mul29 r[3];
};
template <int V>
__global__ __launch_bounds__(kBlock) void k_fold_multi(const uint64_t *in, uint64_t *out, uint64_t n_out, FieldParams P, FoldChallenges ch) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n_out; j += stride) {
        Fe x[1 << V];
#pragma unroll
        for (int c = 0; c < (1 << V); ++c) x[c] = fe_load(in, j + (uint64_t)c * n_out);
#pragma unroll
        for (int lvl = 0; lvl < V; ++lvl) {
#pragma unroll
            for (int c = 0; c < (1 << (V - 1 - lvl)); ++c)
                x[c] = fe_sub(x[c], fe_mul29(fe_sub(x[c], x[c + (1 << (V - 1 - lvl))], P), ch.r[lvl], P), P);
        }
        fe_store(out, j, x[0]);
    }
}

// ---- MultiLinearPolynomial::evaluate, bulk (evaluation_form.rs:83-89): the LOW L variables of the table in one pass ---------
// evaluate() folds variable after variable: n launches (or n/3 three-variable ones), each writing a table the next one reads, and
// all but the first are launch latency.  Folding variables is restriction of a multilinear polynomial, so the table after the
// low L variables (index bits 0..L-1) have been assigned is
//   out[g] = sum_{x < 2^L} in[g * 2^L + x] * eq(point_low, x),   eq(., x) = prod_p (bit p of x ? r_p : 1 - r_p)
// -- the same field elements whatever the order of the folds (exact arithmetic, canonical representatives), so the result of
// evaluate() is bit-identical.  One workgroup produces one out[g] from 2^L CONTIGUOUS elements (L = 8..12: 8-128 KiB):
// thread t owns the elements x = xm * 256 + t, all loaded before any arithmetic; waves 0-2 build three 16-entry eq tables (bits
// 0-3, 4-7, 8-L-1; chains of <= 3 multiplications, hidden under the loads); then each thread adds its <= 16 products
// in[.] * eq_m[xm] UNREDUCED (wide_mac), reduces once, multiplies by its own eq_l[t] = eq_47[t >> 4] * eq_03[t & 15] and the
// workgroup sums.  Per element: one 512-bit product and 32 bytes read; the remaining n - L variables are a 2^L times smaller table.
// what is left after a weighted bulk launch: the sum of its n <= 4096 outputs, one workgroup; result (and the completion word)
// straight into pinned host memory when the caller asks for it
__global__ __launch_bounds__(kBlock) void k_eval_sum(const uint64_t *__restrict__ in, uint32_t n, FieldParams P, uint64_t *__restrict__ out,
                                                     volatile uint32_t *flag, uint32_t seq) {
    __shared__ uint32_t red[kBlock / 64][8];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    Fe acc = fe_zero();
    Fe x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (tid + 256u * i < n) x[i] = fe_load(in, tid + 256u * i);   // all loads first: one memory round trip
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (tid + 256u * i < n) acc = fe_add(acc, x[i], P);
    acc = fe_wave_sum(acc, P);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[tid >> 6][i] = acc.v[i];
    }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < kBlock / 64; ++wv) {
            Fe o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o.v[i] = red[wv][i];
            acc = fe_add(acc, o, P);
        }
        fe_store(out, 0, acc);
        if (flag) {
            __threadfence_system();
            *flag = seq;
        }
    }
}

// Entry j (< 2^nb, nb <= 4) of the eq table over the index bits first .. first + nb - 1 of a point record PT (r[bit][8], Montgomery
// form; first and nb wave-uniform, so the coordinates are scalar loads from the argument segment):
//   (sel_0 * sel_1) * (sel_2 * sel_3),   sel_k = r_k if bit k of j is set, else 1 - r_k;   absent factors are 1
// TWO levels of multiplications, the two of the first level independent of each other (they share the multiplier's issue slots),
// instead of a chain of three: the table build is the head of every evaluate workgroup's dependent chain.  Exact field
// arithmetic: the same canonical entries whatever the association.
template <class PT>
ZK_D Fe eq_entry_depth2(const PT &pt, uint32_t first, uint32_t nb, uint32_t j, const FieldParams &P) {
    Fe one;
#pragma unroll
    for (int i = 0; i < 8; ++i) one.v[i] = P.r1[i];
    Fe f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t idx = (uint32_t)k < nb ? first + k : first;   // (in range even when the factor is absent)
        Fe r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r.v[i] = pt.r[idx][i];
        const Fe sel = (j >> k) & 1 ? r : fe_sub(one, r, P);
        f[k] = (uint32_t)k < nb ? sel : one;
    }
#ifdef ZK_EQ_CHAIN   // A/B builds only: round 4's chain of three dependent multiplications
    return fe_mul(fe_mul(fe_mul(f[0], f[1], P), f[2], P), f[3], P);
#else
    const Fe a = fe_mul(f[0], f[1], P), b = fe_mul(f[2], f[3], P);
    return fe_mul(a, b, P);
#endif
}

constexpr int kEvalLowMax = 12, kEvalLowMin = 8;   // L = 8: one element per thread
struct EvalLowPoint {   // r for index bit p (Montgomery form), p = 0 the least significant bit = the LAST variable
    uint32_t r[kEvalLowMax][8];
};
__global__ __launch_bounds__(kBlock) void k_eval_low(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint32_t L,
                                                     EvalLowPoint pt, FieldParams P, volatile uint32_t *flag, uint32_t seq, EvalHighPoint ph) {
    __shared__ Fe eq[3][16];
    __shared__ Fe wg;   // eq(point_high, blockIdx.x) when the outputs are weighted (ph.n > 0): wave 3, which has no table to build
    __shared__ uint32_t red[kBlock / 64][8];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_m = 1u << (L - 8);   // elements per thread
    const uint64_t base = ((uint64_t)blockIdx.x << L) + tid;
    Fe x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if ((uint32_t)i < n_m) x[i] = fe_load(in, base + (uint64_t)i * 256);
    if (wave < 3) {   // table `wave`: bits 4*wave .. (the third table has L - 8 bits); lane j < 16 builds entry j
        const uint32_t nb = wave < 2 ? 4u : L - 8;
        const Fe acc = eq_entry_depth2(pt, wave < 2 ? 4 * wave : 8u, nb, lane, P);
        if (lane < 16) eq[wave][lane] = acc;
    } else if (ph.n) {
        const Fe f = eval_high_weight(ph, blockIdx.x, lane, P);
        if (lane == eval_high_lane(ph.n)) wg = f;
    }
    __syncthreads();
    WideAcc w;
    wide_zero(w);
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if ((uint32_t)i < n_m) {
            const Fe m = eq[2][i];
            wide_mac(w, x[i].v, m.v);
        }
    const Fe wl = fe_mul(eq[1][tid >> 4], eq[0][tid & 15], P);
    Fe s = fe_mul(redc_wide(w, P), wl, P);
    s = fe_wave_sum(s, P);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[tid >> 6][i] = s.v[i];
    }
    __syncthreads();
    if (tid == 0) {
        Fe acc = s;
        for (int wv = 1; wv < kBlock / 64; ++wv) {
            Fe o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o.v[i] = red[wv][i];
            acc = fe_add(acc, o, P);
        }
        if (ph.n) acc = fe_mul(acc, wg, P);
        fe_store(out, blockIdx.x, acc);
        if (flag) {   // (single-workgroup launches only) completion word for the host, after the result
            __threadfence_system();
            *flag = seq;
        }
    }
}

// ---- MultiLinearPolynomial::evaluate, tail (evaluation_form.rs:83-89) -----------------------------------------------------
// Once the table is small every further fold is launch latency.  One 1024-thread workgroup finishes the last m <= 12
// variables: the first of them is folded while the 2^m elements are read from HBM (so 2^(m-1) elements = 64 KiB of LDS at
// m = 12), the rest in place in LDS with one barrier per variable.  chs: the m remaining assignments, prepared on the host.
constexpr int kEvalTailVars = 12;
constexpr int kEvalTailThreads = 1024;
constexpr int kEvalChWords = 9;
struct EvalTailChallenges {   // the m remaining assignments in prepared form, passed in the kernel arguments (no staging copy)
    uint32_t w[kEvalTailVars][kEvalChWords];
};
__global__ __launch_bounds__(kEvalTailThreads) void k_evaluate_tail(const uint64_t *__restrict__ in, uint32_t m,
                                                                    EvalTailChallenges chs, FieldParams P,
                                                                    uint64_t *__restrict__ out, volatile uint32_t *flag = nullptr, uint32_t seq = 0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ev_smem[];
    uint64_t *T = reinterpret_cast<uint64_t *>(ev_smem);
    const uint32_t tid = threadIdx.x;
    auto load_r = [&](uint32_t v) {   // v is wave-uniform: scalar loads from the argument segment
        Mul29 r;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.l[i] = chs.w[v][i];
        return r;
    };
    uint32_t q = 1u << (m - 1);
    {
        const Mul29 r = load_r(0);
        for (uint32_t j = tid; j < q; j += kEvalTailThreads) {
            const Fe lo = fe_load(in, j), hi = fe_load(in, j + q);
            fe_store(T, j, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));
        }
    }
    __syncthreads();
    for (uint32_t v = 1; v < m; ++v) {
        q >>= 1;
        const Mul29 r = load_r(v);
        for (uint32_t j = tid; j < q; j += kEvalTailThreads) {
            const Fe lo = fe_load(T, j), hi = fe_load(T, j + q);
            fe_store(T, j, fe_sub(lo, fe_mul29(fe_sub(lo, hi, P), r, P), P));   // in place: j and j+q belong to this thread
        }
        __syncthreads();
    }
    if (tid == 0) {
        fe_store(out, 0, fe_load(T, 0));
        if (flag) {   // completion word for the host (host_core.hpp host_flag_wait): after the result, system scope
            __threadfence_system();
            *flag = seq;
        }
    }
}

// ---- ProductPoly::prod_reduce (product_poly.rs:66-74) --------------------------------------------------------
// n >= 64: the fold's wave-coalesced run access (two 1-KiB dwordx4 accesses per 64 elements and table + a DPP half swap, nontemporal:
// every table is streamed once).  Measured at 2^24: 0.62 (k = 2) / 0.57 (k = 3) of the HBM peak with 32 bytes per lane.
__global__ __launch_bounds__(kBlock) void k_prod_reduce_run(FactorPtrs fp, int k, uint64_t n, uint64_t *__restrict__ out, FieldParams P) {
    const uint32_t lane = threadIdx.x & 63;
    const bool odd = lane & 1;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    uint4 *out4 = reinterpret_cast<uint4 *>(out);
    for (uint64_t e0 = wave * 64; e0 < n; e0 += nwaves * 64) {
        const uint64_t c0 = 2 * e0 + lane;
        Fe acc;
        {
            const uint4 *q = reinterpret_cast<const uint4 *>(fp.in[0]);
            acc = pair_gather(nt_load16(q + c0), nt_load16(q + c0 + 64), odd);
        }
        for (int f = 1; f < k; ++f) {
            const uint4 *q = reinterpret_cast<const uint4 *>(fp.in[f]);
            acc = fe_mul_tt(acc, pair_gather(nt_load16(q + c0), nt_load16(q + c0 + 64), odd), P);   // carry-free table x table product
        }
        uint4 oa, ob;
        pair_scatter(acc, odd, oa, ob);
        nt_store16(oa, out4 + c0);
        nt_store16(ob, out4 + c0 + 64);
    }
}
__global__ __launch_bounds__(kBlock) void k_prod_reduce(FactorPtrs fp, int k, uint64_t n, uint64_t *__restrict__ out,
                                                        FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
        Fe acc = fe_load(fp.in[0], j);
        for (int f = 1; f < k; ++f) acc = fe_mul(acc, fe_load(fp.in[f], j), P);
        fe_store(out, j, acc);
    }
}

// ---- MultiLinearPolynomial::to_bytes (evaluation_form.rs:97-103): 32-byte big-endian canonical integers ----------
__global__ __launch_bounds__(kBlock) void k_to_bytes(const uint64_t *__restrict__ in, uint8_t *__restrict__ out,
                                                     uint64_t n, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
        const Fe c = fe_to_canonical(fe_load(in, j), P);
        uint4 *o = reinterpret_cast<uint4 *>(out + 32 * j);
        o[0] = make_uint4(__builtin_bswap32(c.v[7]), __builtin_bswap32(c.v[6]), __builtin_bswap32(c.v[5]),
                          __builtin_bswap32(c.v[4]));
        o[1] = make_uint4(__builtin_bswap32(c.v[3]), __builtin_bswap32(c.v[2]), __builtin_bswap32(c.v[1]),
                          __builtin_bswap32(c.v[0]));
    }
}

// ---- CoeffMultilinearPolynomial::to_evaluation_form (coefficient_form.rs:340-347) ---------------------------------------
// eval[idx] = sum over keys that are subsets of the point's variable set.  With key bit v <-> variable v and table index
// bit (n-1-v) <-> variable v, that is a zeta (subset-sum) transform of the coefficient vector placed at bit-reversed
// positions: scatter, then one in-place pass per variable: T[x | b] += T[x].
// (the round-4 global-pass form, kept behind ZK_ZETA_GLOBAL=1 for A/B; the shipped transform is zeta_kernels.cuh)
__global__ __launch_bounds__(kBlock) void k_scatter_terms(const uint64_t *__restrict__ idx, const uint64_t *__restrict__ coeffs,
                                                          uint64_t n_terms, uint64_t *__restrict__ table) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < n_terms; t += stride)
        fe_store(table, idx[t], fe_load(coeffs, t));   // idx = bit-reversed keys, unique (merged on the host)
}
__global__ __launch_bounds__(kBlock) void k_zeta_pass(uint64_t *table, uint64_t pairs, uint32_t pos, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < pairs; j += stride) {
        const uint64_t lo = insert_zero_bit(j, pos), hi = lo | (1ull << pos);
        fe_store(table, hi, fe_add(fe_load(table, hi), fe_load(table, lo), P));
    }
}

// V consecutive bit positions pos .. pos+V-1 in one pass: a thread owns the 2^V elements that differ in those bits, applies the V
// levels of the subset-sum butterfly (hi += lo: additions only) in registers and writes the 2^V - 1 elements that changed --
// a third of the launches and 0.4 of the traffic of three single passes at V = 3.
template <int V>
__global__ __launch_bounds__(kBlock) void k_zeta_multi(uint64_t *table, uint64_t groups, uint32_t pos, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t low_mask = (1ull << pos) - 1;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += stride) {
        const uint64_t base = ((g >> pos) << (pos + V)) | (g & low_mask);
        Fe x[1 << V];
#pragma unroll
        for (int c = 0; c < (1 << V); ++c) x[c] = fe_load(table, base | ((uint64_t)c << pos));
#pragma unroll
        for (int b = 0; b < V; ++b)
#pragma unroll
            for (int c = 0; c < (1 << V); ++c)
                if (c & (1 << b)) x[c] = fe_add(x[c], x[c ^ (1 << b)], P);
#pragma unroll
        for (int c = 1; c < (1 << V); ++c) fe_store(table, base | ((uint64_t)c << pos), x[c]);
    }
}

// ---- synthetic inputs: element i = first hash(seed, i, attempt) < p, stored in Montgomery form --------
ZK_D uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(kBlock) void k_fill_random(uint64_t *__restrict__ out, uint64_t n, uint64_t seed,
                                                        uint64_t first, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint32_t topbits = P.bits & 31u;
    const uint32_t topmask = topbits ? ((1u << topbits) - 1u) : 0xffffffffu;
    const int toplimb = (int)((P.bits + 31u) / 32u) - 1;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
        const uint64_t h0 = splitmix64(seed ^ splitmix64(first + j));
        Fe c;
        for (uint64_t attempt = 0;; ++attempt) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint64_t x = splitmix64(h0 + 4 * attempt + (uint64_t)w);
                c.v[2 * w] = (uint32_t)x;
                c.v[2 * w + 1] = (uint32_t)(x >> 32);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i == toplimb) c.v[i] &= topmask;
                else if (i > toplimb) c.v[i] = 0;
            }
            Fe d;
            if (sub8(d.v, c.v, P.p)) break;   // borrow => c < p
        }
        fe_store(out, j, fe_from_canonical(c, P));
    }
}

// ---- PartialEq on tables: any differing 16-byte word raises the flag ------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_compare(const uint4 *__restrict__ a, const uint4 *__restrict__ b, uint64_t n16,
                                                    uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    bool diff = false;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n16; j += stride) {
        const uint4 x = a[j], y = b[j];
        diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
    }
    if (diff) atomicOr(flag, 1u);
}

// ---- measurement kernels -----------------------------------------------------------------------------------------
// dependent fe_mul chain entirely in registers: 2 independent chains per thread
__global__ __launch_bounds__(kBlock) void k_bench_modmul(uint64_t *__restrict__ out, int iters, FieldParams P, Fe seed, Mul29 c29,
                                                         int variant) {
    Fe a = seed, b = seed;
    a.v[0] ^= threadIdx.x;
    b.v[1] ^= blockIdx.x + 7u * threadIdx.x;   // both chains per-lane (a uniform chain would be scalarised)
    a = fe_from_canonical(fe_to_canonical(a, P), P);
    if (variant == 0) {          // saturated Montgomery product of two variable operands
        for (int i = 0; i < iters; ++i) {
            a = fe_mul(a, b, P);
            b = fe_mul(b, a, P);
        }
    } else {                     // unsaturated product by a prepared (wave-uniform) operand
        for (int i = 0; i < iters; ++i) {
            a = fe_mul29(a, c29, P);
            b = fe_mul29(b, c29, P);
        }
    }
    if (a.v[0] == 0x12345678u && b.v[3] == 0x9abcdef0u) fe_store(out, 0, a);   // keep the chain live
}
__global__ __launch_bounds__(kBlock) void k_bench_copy(const uint4 *__restrict__ in, uint4 *__restrict__ out, uint64_t n16) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n16; j += stride) out[j] = in[j];
}

}  // namespace zk
