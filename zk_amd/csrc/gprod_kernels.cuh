// gprod_kernels.cuh -- gfx950 kernels of the grand-product argument (no reference item; definition: tests/gprod_ref.py; host side: gprod.hip;
// DESIGN.md section 17).
//
// The product tree over V_n = t + sigma: V_j[i] = V_{j+1}[i] V_{j+1}[i + 2^j], the low half times the high half, kept as a heap
// (heap[2^j + i] = V_j[i], heap[0] = 1).  A level's two operands are 2^j elements apart, so taking level m + A down to level m reads, for
// i < M = 2^m, the 2^A elements i + s M: 2^A coalesced streams, the access pattern of k_fri_fold<A> (fri_kernels.cuh).  k_ptree<A>
// multiplies them down A levels in registers and writes the 2^(A-1) + .. + 1 results to their levels' slots of the heap: one
// multiplication per output, and with A = 3 the whole tree reads about 1.14 x 2^n elements against 2 x 2^n one level per launch.  The
// first launch adds sigma as it reads, so t + sigma is never written.  From 2^kPtreeLdsVars elements down one workgroup finishes out of
// LDS (k_ptree_lds): the levels there are launch-bound, not bandwidth-bound.
//
// k_gprod_chain / k_gprod_finish are the scalar steps between the layers' sumchecks, one wave each, after k_gkr_chain_* (gkr_kernels.cuh):
// the transcript never leaves the device.
#pragma once
#include "common.cuh"
#include "transcript.cuh"

namespace zk {

constexpr uint32_t kPtreeLdsVars = 10;    // k_ptree_lds takes a level of at most 2^10 elements (its half, 16 KiB, sits in LDS)
constexpr uint32_t kPtreeMaxFuse = 3;     // levels per fused launch: 2^3 input elements and 7 products of 8 VGPRs each in registers
constexpr uint32_t kPtreeFuseDefault = 3;

// x[0 .. 2^L) <- x[s] x[s + 2^L], stored as level m + L of the heap (elements e0 + s M of it, the wave's run), down to L = 0
// (the level as a template parameter: every index into x is a constant, so nothing goes to scratch)
template <int L>
ZK_D void ptree_levels(Fe *x, uint64_t *__restrict__ heap, uint32_t m, uint64_t e0, uint32_t lane, const FieldParams &P) {
    const uint64_t M = 1ull << m;
#pragma unroll
    for (int s = 0; s < (1 << L); ++s) {
        x[s] = fe_mul_tt(x[s], x[s + (1 << L)], P);
        uint64_t *run = heap + 4 * ((M << L) + e0 + (uint64_t)s * M);
        if (L == 0) run_store(run, lane, x[s]);   // the next launch reads it
        else run_store_nt(run, lane, x[s]);       // read again only by the layer's sumcheck, after the rest of the tree
    }
    if constexpr (L > 0) ptree_levels<L - 1>(x, heap, m, e0, lane, P);
}
// level m + A (src: 2^(m+A) elements; SHIFT: plus sigma) -> levels m + A - 1 .. m of the heap.  M = 2^m is a multiple of 64: a wave moves
// runs of 64 consecutive elements of each stream (common.cuh run_load_nt), lane l owning the same element of every stream and output.
template <int A, bool SHIFT>
__global__ __launch_bounds__(kBlock) void k_ptree(const uint64_t *__restrict__ src, uint64_t *__restrict__ heap, uint32_t m, Fe sigma, FieldParams P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t M = 1ull << m, wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t e0 = wave * 64; e0 < M; e0 += nwaves * 64) {
        Fe x[1 << A];
#pragma unroll
        for (int s = 0; s < (1 << A); ++s) {
            x[s] = run_load_nt(src + 4 * (e0 + (uint64_t)s * M), lane);
            if (SHIFT) x[s] = fe_add(x[s], sigma, P);
        }
        ptree_levels<A - 1>(x, heap, m, e0, lane, P);
    }
}
// One workgroup: level v <= kPtreeLdsVars (src: 2^v elements; shift: plus sigma) -> levels v - 1 .. 0 of the heap, and heap[0] = 1.
// Level j overwrites the low half of level j + 1 in LDS: thread i reads slots i and i + 2^j and writes slot i, and no other thread
// touches slot i < 2^j in that step.
__global__ __launch_bounds__(kBlock) void k_ptree_lds(const uint64_t *__restrict__ src, uint64_t *__restrict__ heap, uint32_t v, uint32_t shift, Fe sigma,
                                                      FieldParams P) {
    __shared__ Fe lvl[1u << (kPtreeLdsVars - 1)];
    const uint32_t half = 1u << (v - 1);
    for (uint32_t i = threadIdx.x; i < half; i += kBlock) {
        Fe a = fe_load(src, i), b = fe_load(src, i + half);
        if (shift) {
            a = fe_add(a, sigma, P);
            b = fe_add(b, sigma, P);
        }
        const Fe q = fe_mul_tt(a, b, P);
        lvl[i] = q;
        fe_store(heap, half + i, q);
    }
    for (uint32_t h = half >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < h; i += kBlock) {
            const Fe q = fe_mul_tt(lvl[i], lvl[i + h], P);
            lvl[i] = q;
            fe_store(heap, h + i, q);
        }
    }
    if (threadIdx.x == 0) fe_store(heap, 0, fe_one(P));
}
// out[i] = t[i] + sigma (the top layer's sumcheck folds V_n, which the tree never writes; only when sigma != 0)
__global__ __launch_bounds__(kBlock) void k_gprod_shift(const uint64_t *__restrict__ t, uint64_t *__restrict__ out, uint64_t n, Fe sigma, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) fe_store(out, i, fe_add(fe_load(t, i), sigma, P));
}

// ---- the proof's transcript on the device (one wave per step) --------------------------------------------------------------------------
// The end of layer j.  ab = [a, b] = V_{j+1}(0, rho), V_{j+1}(1, rho): the sumcheck's factor values, or V_1 itself at j = 0.  proof_ab gets
// them; absorb a, b; tau; pt_next[0] = tau (the sumcheck wrote rho behind it: r_{j+1} = (tau, rho)); c_{j+1} = a + tau (b - a), kept at
// `claim` and absorbed as the next sumcheck's first message (after the last layer nobody reads the transcript again).
// FIRST (layer 0): c_0 = P (heap[1]) is absorbed in front.
template <bool FIRST>
__global__ __launch_bounds__(64) void k_gprod_chain(WordSponge *__restrict__ gsp, const uint64_t *__restrict__ product, const uint64_t *__restrict__ ab,
                                                     uint64_t *__restrict__ proof_ab, uint64_t *__restrict__ pt_next, uint64_t *__restrict__ claim,
                                                     FieldParams P) {
    __shared__ Fe buf[4];
    const LaneKeccak L = lane_keccak_init();
    LaneSponge sp = lane_sponge_load(gsp, L);
    const Fe a = fe_load(ab, 0), b = fe_load(ab, 1);   // wave-uniform
    if (L.lane == 0) {
        if (FIRST) buf[0] = fe_load(product, 0);
        buf[1] = a;
        buf[2] = b;
        fe_store(proof_ab, 0, a);
        fe_store(proof_ab, 1, b);
    }
    __syncthreads();
    lane_absorb_elems(sp, L, FIRST ? buf : buf + 1, FIRST ? 3 : 2, P);
    Mul29 t29;
    const Fe tau = lane_squeeze(sp, L, P, t29);
    const Fe c = fe_add(a, fe_mul(tau, fe_sub(b, a, P), P), P);
    if (L.lane == 0) {
        buf[3] = c;
        fe_store(pt_next, 0, tau);
        fe_store(claim, 0, c);
    }
    __syncthreads();
    lane_absorb_elems(sp, L, buf + 3, 1, P);
    lane_sponge_store(gsp, sp, L);
}
// the proof block's tail behind the 2 n^2 proof elements: [P | r_n (n elements) | c_n - sigma]
__global__ __launch_bounds__(64) void k_gprod_finish(const uint64_t *__restrict__ product, const uint64_t *__restrict__ point, const uint64_t *__restrict__ claim,
                                                      uint32_t n, Fe sigma, uint64_t *__restrict__ tail, FieldParams P) {
    const uint32_t lane = threadIdx.x;
    if (lane == 0) {
        fe_store(tail, 0, fe_load(product, 0));
        fe_store(tail, 1 + n, fe_sub(fe_load(claim, 0), sigma, P));
    }
    if (lane < n) fe_store(tail, 1 + lane, fe_load(point, lane));
}

}  // namespace zk
