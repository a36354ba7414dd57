// fsum_kernels.cuh -- gfx950 kernels of the fractional-sum (LogUp) argument and of the lookup multiplicities (no reference item; definition:
// tests/fsum_ref.py; host side: fsum.hip).
//
// The fraction tree over P_n = p (or all ones), Q_n = q + sigma: P_j[i] = P_{j+1}[i] Q_{j+1}[i + 2^j] + P_{j+1}[i + 2^j] Q_{j+1}[i],
// Q_j[i] = Q_{j+1}[i] Q_{j+1}[i + 2^j] -- the sum of the two fractions under a node, never divided out -- kept as two heaps
// (heap[2^j + i] = level j; heapP[0] = 0, heapQ[0] = 1).  The access pattern is k_ptree's (gprod_kernels.cuh): taking level m + A down to
// level m reads, for i < M = 2^m, the 2^A elements i + s M of each heap -- 2^A coalesced streams per heap -- and k_ftree<A> takes them down
// A levels in registers: three multiplications per node.  PONES: the first launch reads no p stream (its first level is P = Q0 + Q1, no
// multiplication); SHIFT: sigma is added to q as it is read, so q + sigma is never written by the tree.  Both heaps live in registers at
// once -- twice k_ptree's pressure -- so kFtreeMaxFuse is what compiles without scratch (profiles/fsum_resource_usage.md).  From
// 2^kFtreeLdsVars elements down one workgroup finishes out of LDS (k_ftree_lds).
//
// k_fsum_chain / k_fsum_finish are the scalar steps between the layers' sumchecks, one wave each, after k_gprod_chain.
//
// The multiplicities m[j] = #{i : witness[i] = table[j]} come from an open-addressing table of 2^(m+1) 32-bit slots (0 = empty, else
// index + 1) over the full 256-bit keys: k_mult_insert (atomics only), k_mult_count (a later launch: plain loads of the slots),
// k_mult_finish (counters -> field elements).  Every probe loop is bounded by the capacity; no thread waits for another.
#pragma once
#include "common.cuh"
#include "transcript.cuh"

namespace zk {

// k_ftree_lds takes a level of at most 2^10 elements of each heap: its halves of P and Q sit beside each other in LDS, 2 x 16 KiB.  One
// more level would be 64 KiB, the whole static allocation a kernel may have; and with the same constant as kPtreeLdsVars the Q heap's
// launches are k_ptree's launches, level for level.
constexpr uint32_t kFtreeLdsVars = 10;
constexpr uint32_t kFtreeMaxFuse = 2;     // levels per fused launch: 2 x 2^2 input elements of 8 VGPRs each in registers (A = 3 spills)
constexpr uint32_t kFtreeFuseDefault = 2;
constexpr uint32_t kMultMaxTableVars = 30, kMultMaxWitnessVars = 31;   // index + 1 and a count both fit 32 bits

// level m + L + 1 in xp / xq[0 .. 2^(L+1)) -> level m + L in xp / xq[0 .. 2^L), stored to the heaps (elements e0 + s M of the level, the
// wave's run), down to L = 0.  ONES: the level above has P = 1 everywhere (xp is not read).  The level is a template parameter: every
// index into xp / xq is a constant, so nothing goes to scratch.
template <int L, bool ONES>
ZK_D void ftree_levels(Fe *xp, Fe *xq, uint64_t *__restrict__ heap_p, uint64_t *__restrict__ heap_q, uint32_t m, uint64_t e0, uint32_t lane,
                       const FieldParams &P) {
    const uint64_t M = 1ull << m;
#pragma unroll
    for (int s = 0; s < (1 << L); ++s) {
        const Fe q0 = xq[s], q1 = xq[s + (1 << L)];
        if (ONES) xp[s] = fe_add(q0, q1, P);
        else xp[s] = fe_add(fe_mul_tt(xp[s], q1, P), fe_mul_tt(xp[s + (1 << L)], q0, P), P);
        xq[s] = fe_mul_tt(q0, q1, P);
        const uint64_t at = 4 * ((M << L) + e0 + (uint64_t)s * M);
        if (L == 0) {   // the next launch reads it
            run_store(heap_p + at, lane, xp[s]);
            run_store(heap_q + at, lane, xq[s]);
        } else {        // read again only by the layer's sumcheck, after the rest of the tree
            run_store_nt(heap_p + at, lane, xp[s]);
            run_store_nt(heap_q + at, lane, xq[s]);
        }
    }
    if constexpr (L > 0) ftree_levels<L - 1, false>(xp, xq, heap_p, heap_q, m, e0, lane, P);
}
// level m + A (src_p, src_q: 2^(m+A) elements each; PONES: no src_p, P = 1; SHIFT: q plus sigma) -> levels m + A - 1 .. m of both heaps.
// M = 2^m is a multiple of 64: a wave moves runs of 64 consecutive elements of each stream, lane l owning the same element of every one.
template <int A, bool PONES, bool SHIFT>
__global__ __launch_bounds__(kBlock) void k_ftree(const uint64_t *__restrict__ src_p, const uint64_t *__restrict__ src_q, uint64_t *__restrict__ heap_p,
                                                  uint64_t *__restrict__ heap_q, uint32_t m, Fe sigma, FieldParams P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t M = 1ull << m, wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t e0 = wave * 64; e0 < M; e0 += nwaves * 64) {
        Fe xp[1 << A], xq[1 << A];
#pragma unroll
        for (int s = 0; s < (1 << A); ++s) {
            xq[s] = run_load_nt(src_q + 4 * (e0 + (uint64_t)s * M), lane);
            if (SHIFT) xq[s] = fe_add(xq[s], sigma, P);
            if (!PONES) xp[s] = run_load_nt(src_p + 4 * (e0 + (uint64_t)s * M), lane);
        }
        ftree_levels<A - 1, PONES>(xp, xq, heap_p, heap_q, m, e0, lane, P);
    }
}
// One workgroup: level v <= kFtreeLdsVars (src_p, src_q: 2^v elements each; ones: P = 1, src_p is not read; shift: q plus sigma) -> levels
// v - 1 .. 0 of both heaps, heapP[0] = 0 and heapQ[0] = 1.  Level j overwrites the low half of level j + 1 in LDS: thread i reads slots i
// and i + 2^j and writes slot i, and no other thread touches slot i < 2^j in that step.
__global__ __launch_bounds__(kBlock) void k_ftree_lds(const uint64_t *__restrict__ src_p, const uint64_t *__restrict__ src_q, uint64_t *__restrict__ heap_p,
                                                      uint64_t *__restrict__ heap_q, uint32_t v, uint32_t ones, uint32_t shift, Fe sigma, FieldParams P) {
    __shared__ Fe lp[1u << (kFtreeLdsVars - 1)], lq[1u << (kFtreeLdsVars - 1)];
    const uint32_t half = 1u << (v - 1);
    for (uint32_t i = threadIdx.x; i < half; i += kBlock) {
        Fe q0 = fe_load(src_q, i), q1 = fe_load(src_q, i + half);
        if (shift) {
            q0 = fe_add(q0, sigma, P);
            q1 = fe_add(q1, sigma, P);
        }
        const Fe pn = ones ? fe_add(q0, q1, P) : fe_add(fe_mul_tt(fe_load(src_p, i), q1, P), fe_mul_tt(fe_load(src_p, i + half), q0, P), P);
        const Fe qn = fe_mul_tt(q0, q1, P);
        lp[i] = pn;
        lq[i] = qn;
        fe_store(heap_p, half + i, pn);
        fe_store(heap_q, half + i, qn);
    }
    for (uint32_t h = half >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < h; i += kBlock) {
            const Fe q0 = lq[i], q1 = lq[i + h];
            const Fe pn = fe_add(fe_mul_tt(lp[i], q1, P), fe_mul_tt(lp[i + h], q0, P), P), qn = fe_mul_tt(q0, q1, P);
            lp[i] = pn;
            lq[i] = qn;
            fe_store(heap_p, h + i, pn);
            fe_store(heap_q, h + i, qn);
        }
    }
    if (threadIdx.x == 0) {
        fe_store(heap_p, 0, fe_zero());
        fe_store(heap_q, 0, fe_one(P));
    }
}
// out[i] = t[i] + sigma (the top layer's sumcheck folds Q_n, which the tree never writes; only when sigma != 0)
__global__ __launch_bounds__(kBlock) void k_fsum_shift(const uint64_t *__restrict__ t, uint64_t *__restrict__ out, uint64_t n, Fe sigma, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) fe_store(out, i, fe_add(fe_load(t, i), sigma, P));
}
// out[i] = 1 (the top level's P when p is not given: its two halves are the top layer's constant tables)
__global__ __launch_bounds__(kBlock) void k_fsum_ones(uint64_t *__restrict__ out, uint64_t n, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const Fe one = fe_one(P);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) fe_store(out, i, one);
}
// s[i] = p1[i] + lambda q1[i], lambda in device memory: p0 q1 + p1 q0 + lambda q0 q1 = p0 q1 + s q0, two products of three tables with E
__global__ __launch_bounds__(kBlock) void k_fsum_comb(const uint64_t *__restrict__ p1, const uint64_t *__restrict__ q1, const uint64_t *__restrict__ lambda,
                                                      uint64_t *__restrict__ s, uint64_t n, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const Fe lam = fe_load(lambda, 0);   // wave-uniform
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        fe_store(s, i, fe_add(fe_load(p1, i), fe_mul(lam, fe_load(q1, i), P), P));
}

// ---- the proof's transcript on the device (one wave per step) --------------------------------------------------------------------------
// The end of layer j and the start of layer j + 1.  FIRST (layer 0): `a` = level 1 of P, `b` = level 1 of Q (two elements each: p0, p1 and
// q0, q1), and N = sum_p[0], D = sum_q[0] are absorbed in front.  Otherwise `a` = the sumcheck's factor values (E, P0, Q1 | E', S, Q0 at
// rho): p0 = a[1], q1 = a[2], s = a[4], q0 = a[5], and p1 = s - lambda q1 with this layer's lambda (state[2]).  proof4 gets p0, p1, q0, q1;
// they are absorbed; tau; pt_next[0] = tau (the sumcheck wrote rho behind it: r_{j+1} = (tau, rho)); state[0], state[1] = cP_{j+1}, cQ_{j+1} =
// p0 + tau (p1 - p0), q0 + tau (q1 - q0); then layer j + 1's lambda -> state[2], and cP + lambda cQ absorbed as its sumcheck's first
// message (after the last layer nobody reads the transcript again).
template <bool FIRST>
__global__ __launch_bounds__(64) void k_fsum_chain(WordSponge *__restrict__ gsp, const uint64_t *__restrict__ a, const uint64_t *__restrict__ b,
                                                   const uint64_t *__restrict__ sum_p, const uint64_t *__restrict__ sum_q, uint64_t *__restrict__ proof4,
                                                   uint64_t *__restrict__ pt_next, uint64_t *__restrict__ state, FieldParams P) {
    __shared__ Fe buf[7];
    const LaneKeccak L = lane_keccak_init();
    LaneSponge sp = lane_sponge_load(gsp, L);
    Fe p0, p1, q0, q1;   // wave-uniform
    if (FIRST) {
        p0 = fe_load(a, 0), p1 = fe_load(a, 1), q0 = fe_load(b, 0), q1 = fe_load(b, 1);
    } else {
        p0 = fe_load(a, 1), q1 = fe_load(a, 2), q0 = fe_load(a, 5);
        p1 = fe_sub(fe_load(a, 4), fe_mul(fe_load(state, 2), q1, P), P);
    }
    if (L.lane == 0) {
        if (FIRST) buf[0] = fe_load(sum_p, 0), buf[1] = fe_load(sum_q, 0);
        buf[2] = p0, buf[3] = p1, buf[4] = q0, buf[5] = q1;
        fe_store(proof4, 0, p0);
        fe_store(proof4, 1, p1);
        fe_store(proof4, 2, q0);
        fe_store(proof4, 3, q1);
    }
    __syncthreads();
    lane_absorb_elems(sp, L, FIRST ? buf : buf + 2, FIRST ? 6 : 4, P);
    Mul29 t29;
    const Fe tau = lane_squeeze(sp, L, P, t29);
    const Fe cp = fe_add(p0, fe_mul(tau, fe_sub(p1, p0, P), P), P), cq = fe_add(q0, fe_mul(tau, fe_sub(q1, q0, P), P), P);
    const Fe lam = lane_squeeze(sp, L, P, t29);
    if (L.lane == 0) {
        buf[6] = fe_add(cp, fe_mul(lam, cq, P), P);
        fe_store(pt_next, 0, tau);
        fe_store(state, 0, cp);
        fe_store(state, 1, cq);
        fe_store(state, 2, lam);
    }
    __syncthreads();
    lane_absorb_elems(sp, L, buf + 6, 1, P);
    lane_sponge_store(gsp, sp, L);
}
// the proof block's tail behind the 2 n^2 + 2 n proof elements: [N | D | r_n (n elements) | cP_n | cQ_n - sigma]
__global__ __launch_bounds__(64) void k_fsum_finish(const uint64_t *__restrict__ sum_p, const uint64_t *__restrict__ sum_q, const uint64_t *__restrict__ point,
                                                    const uint64_t *__restrict__ state, uint32_t n, Fe sigma, uint64_t *__restrict__ tail, FieldParams P) {
    const uint32_t lane = threadIdx.x;
    if (lane == 0) {
        fe_store(tail, 0, fe_load(sum_p, 0));
        fe_store(tail, 1, fe_load(sum_q, 0));
        fe_store(tail, 2 + n, fe_load(state, 0));
        fe_store(tail, 3 + n, fe_sub(fe_load(state, 1), sigma, P));
    }
    if (lane < n) fe_store(tail, 2 + lane, fe_load(point, lane));
}

// ---- lookup multiplicities ---------------------------------------------------------------------------------------------------------------
struct MultKey {
    uint4 lo, hi;   // the 8 Montgomery limb words
};
ZK_D MultKey mult_key(const uint64_t *__restrict__ t, uint64_t i) {
    const uint4 *q = reinterpret_cast<const uint4 *>(t + 4 * i);
    return MultKey{q[0], q[1]};
}
ZK_D bool mult_key_eq(const MultKey &x, const MultKey &y) {
    return x.lo.x == y.lo.x && x.lo.y == y.lo.y && x.lo.z == y.lo.z && x.lo.w == y.lo.w && x.hi.x == y.hi.x && x.hi.y == y.hi.y && x.hi.z == y.hi.z &&
           x.hi.w == y.hi.w;
}
// every word goes through a multiply and a xor-shift (the 32-bit finaliser of MurmurHash3 between the words): keys that differ in one
// word, the lowest or the highest, land in unrelated slots.  Only the speed depends on it, never the result.
ZK_D uint32_t mult_hash(const MultKey &k) {
    const uint32_t w[8] = {k.lo.x, k.lo.y, k.lo.z, k.lo.w, k.hi.x, k.hi.y, k.hi.z, k.hi.w};
    uint32_t h = 0x9E3779B9u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h ^= w[i];
        h ^= h >> 16;
        h *= 0x85EBCA6Bu;
        h ^= h >> 13;
        h *= 0xC2B2AE35u;
        h ^= h >> 16;
    }
    return h;
}
// counters: [missing | first_missing | duplicates] (u64 each)
// One thread per table entry: linear probing from the key's hash.  The slots are touched by atomics only (another XCD's plain store might
// not be seen inside the launch); the keys are the caller's table, which nobody writes.  A slot never goes back to empty and an equal key
// stops at the first slot that holds its value, so every value has one slot, and the lowest index among equal values stays in it
// (atomicMin) whatever the order of arrival.  At most `cap` probes: half the slots stay empty, so the loop ends long before.
__global__ __launch_bounds__(kBlock) void k_mult_insert(const uint64_t *__restrict__ table, uint64_t n, uint32_t *slots, uint32_t log_cap,
                                                        unsigned long long *counters) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, cap = 1ull << log_cap;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
        const MultKey key = mult_key(table, j);
        uint64_t at = mult_hash(key) & (cap - 1);
        for (uint64_t probes = 0; probes < cap; ++probes, at = (at + 1) & (cap - 1)) {
            const uint32_t old = atomicCAS(slots + at, 0u, (uint32_t)j + 1);
            if (old == 0) break;
            if (mult_key_eq(mult_key(table, old - 1), key)) {
                atomicMin(slots + at, (uint32_t)j + 1);
                atomicAdd(counters + 2, 1ull);
                break;
            }
        }
    }
}
// One thread per witness entry on a capped grid (the loop's trip count is wave-uniform: the ballots below need every lane).  A hit adds
// 1 to the u32 counter of the slot's index: the lanes that agree with the wave's first hit add once together (all lanes when every
// witness entry is equal), the others one by one.  An empty slot: the entry is in no table row.
__global__ __launch_bounds__(kBlock) void k_mult_count(const uint64_t *__restrict__ table, const uint64_t *__restrict__ witness, uint64_t n,
                                                       const uint32_t *__restrict__ slots, uint32_t log_cap, uint32_t *counts, unsigned long long *counters) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, cap = 1ull << log_cap;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t i = base + lane;
        bool hit = false;
        uint32_t idx = 0;
        if (i < n) {
            const MultKey key = mult_key(witness, i);
            uint64_t at = mult_hash(key) & (cap - 1);
            bool missing = true;   // (a full table cannot happen: at most cap / 2 slots are taken)
            for (uint64_t probes = 0; probes < cap; ++probes, at = (at + 1) & (cap - 1)) {
                const uint32_t v = slots[at];
                if (v == 0) break;
                if (mult_key_eq(mult_key(table, v - 1), key)) {
                    hit = true, missing = false, idx = v - 1;
                    break;
                }
            }
            if (missing) {
                atomicAdd(counters + 0, 1ull);
                atomicMin(counters + 1, (unsigned long long)i);
            }
        }
        const uint64_t hits = __ballot(hit);
        if (hits) {
            const int leader = __ffsll((long long)hits) - 1;
            const uint32_t lidx = (uint32_t)__shfl((int)idx, leader);
            const bool same = hit && idx == lidx;
            const uint64_t group = __ballot(same);
            if ((int)lane == leader) atomicAdd(counts + lidx, (uint32_t)__popcll(group));
            if (hit && !same) atomicAdd(counts + idx, 1u);
        }
    }
}
// m[j] = counts[j] as a field element (Montgomery form)
__global__ __launch_bounds__(kBlock) void k_mult_finish(const uint32_t *__restrict__ counts, uint64_t n, uint64_t *__restrict__ m, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) fe_store(m, j, fe_from_u32(counts[j], P));
}

}  // namespace zk
