// inv_kernels.cuh -- batch inversion and running products over tables of field elements (no reference item; definition:
// tests/batch_inverse_ref.py; host side inv.hip; design DESIGN.md section 12).
//
// Batch inversion is Montgomery's trick: the product of a group with its zeros replaced by one is inverted ONCE and peeled back, so n
// inverses cost one field inversion (fe_inverse_binary, inv_field.cuh, on one lane) and about 4 multiplications per element.
// Which elements share a group does not matter, so thread t of a chunk takes the elements base + q * kBlock + t: every load and store
// of a wave is one run of 64 consecutive 32-byte elements.  A zero denominator is written as zero and counted (ark-ff's
// batch_inversion skips zeros); it is replaced by one with a select, not a branch, so zeros cost what other values cost.
#pragma once
#include "common.cuh"
#include "inv_field.cuh"
#include "inv_tree.cuh"

namespace zk {

// elements per thread and per workgroup.  E = 8 holds the 8 inputs and 8 prefixes of the back-substitution in registers without scratch
// (profiles/batch_inverse_resource_usage.md); tests/batch_inverse_ref.py CHUNK mirrors kInvChunk.
constexpr uint32_t kInvPerThread = 8;
constexpr uint32_t kInvChunk = kBlock * kInvPerThread;

// t[i] + shift with a zero replaced by one; *zero says which it was.  i >= n reads nothing and counts as one.
ZK_D Fe inv_load(const uint64_t *v, uint64_t i, uint64_t n, const Fe &shift, const Fe &one, const FieldParams &P, bool *zero) {
    if (i >= n) {
        *zero = false;
        return one;
    }
    const Fe x = fe_add(fe_load(v, i), shift, P);
    *zero = fe_is_zero(x);
    return *zero ? one : x;
}

// launch 1 of 3: totals[c] = the product of chunk c (zeros as one), zeros[c] = how many zeros it holds
__global__ __launch_bounds__(kBlock) void k_inv_chunk_products(const uint64_t *__restrict__ v, uint64_t n, Fe shift, FieldParams P,
                                                               uint64_t *__restrict__ totals, uint32_t *__restrict__ zeros) {
    __shared__ Fe node[2 * kBlock];
    __shared__ uint32_t n_zero;
    if (threadIdx.x == 0) n_zero = 0;
    const uint64_t base = (uint64_t)blockIdx.x * kInvChunk + threadIdx.x;
    const Fe one = fe_one(P);
    Fe acc = one;
    uint32_t nz = 0;
#pragma unroll
    for (uint32_t q = 0; q < kInvPerThread; ++q) {
        bool z;
        const Fe x = inv_load(v, base + (uint64_t)q * kBlock, n, shift, one, P, &z);
        nz += z;
        acc = q ? fe_mul_tt(acc, x, P) : x;
    }
    inv_tree_up(acc, node, P);   // (its first barrier also orders n_zero = 0 before the atomics)
    if (nz) atomicAdd(&n_zero, nz);
    __syncthreads();
    if (threadIdx.x == 0) {
        fe_store(totals, blockIdx.x, node[1]);
        zeros[blockIdx.x] = n_zero;
    }
}
// launch 2 of 3, one workgroup: inv[c] = 1 / totals[c] for the nc chunk products (none of them is zero) -- the same trick one level
// up, thread t taking the run of `per` consecutive chunks from t * per, with the call's only field inversion -- and *zero_count =
// the sum of zeros[].  inv[] holds the run's prefixes in between.
__global__ __launch_bounds__(kBlock) void k_inv_totals(const uint64_t *__restrict__ totals, uint64_t nc, FieldParams P,
                                                       uint64_t *__restrict__ inv, const uint32_t *__restrict__ zeros,
                                                       uint64_t *__restrict__ zero_count) {
    __shared__ Fe node[2 * kBlock];
    __shared__ unsigned long long n_zero;
    if (threadIdx.x == 0) n_zero = 0;
    const uint64_t per = (nc + kBlock - 1) / kBlock, j0 = threadIdx.x * per, j1 = j0 + per < nc ? j0 + per : nc;
    Fe acc = fe_one(P);
    unsigned long long nz = 0;
    for (uint64_t j = j0; j < j1; ++j) {
        fe_store(inv, j, acc);
        acc = fe_mul_tt(acc, fe_load(totals, j), P);
        nz += zeros[j];
    }
    inv_tree_up(acc, node, P);
    if (nz) atomicAdd(&n_zero, nz);
    if (threadIdx.x == 0) node[1] = fe_inverse_binary(node[1], P);
    Fe back = inv_tree_down(node, P);
    for (uint64_t j = j1; j-- > j0;) {
        fe_store(inv, j, fe_mul_tt(back, fe_load(inv, j), P));
        back = fe_mul_tt(back, fe_load(totals, j), P);
    }
    if (threadIdx.x == 0) *zero_count = n_zero;   // (inv_tree_down's barriers are behind every atomic)
}
// launch 3 of 3 (ALONE = false): out[i] = 1 / (v[i] + shift) over chunk blockIdx.x given inv[blockIdx.x] = the inverse of its product;
// ALONE = true is the whole call in one launch for n <= kInvChunk: the workgroup inverts its product itself and writes the count.
// Every thread has its kInvPerThread inputs in registers before its first store and touches no other thread's elements, so out may
// be v (neither is __restrict__).
template <bool ALONE>
__global__ __launch_bounds__(kBlock) void k_inv_apply(const uint64_t *v, uint64_t n, Fe shift, FieldParams P, const uint64_t *__restrict__ inv,
                                                      uint64_t *out, uint64_t *__restrict__ zero_count) {
    __shared__ Fe node[2 * kBlock];
    __shared__ uint32_t n_zero;
    if (ALONE && threadIdx.x == 0) n_zero = 0;
    const uint64_t base = (uint64_t)blockIdx.x * kInvChunk + threadIdx.x;
    const Fe one = fe_one(P);
    Fe x[kInvPerThread], pre[kInvPerThread];   // pre[q] = x[0] ... x[q-1]
    Fe acc = one;
    uint32_t zmask = 0;
    inv_static_for<0, kInvPerThread>([&](auto qc) {
        constexpr uint32_t q = decltype(qc)::value;
        bool z;
        x[q] = inv_load(v, base + (uint64_t)q * kBlock, n, shift, one, P, &z);
        zmask |= (uint32_t)z << q;
        pre[q] = acc;
        acc = q ? fe_mul_tt(acc, x[q], P) : x[q];
    });
    inv_tree_up(acc, node, P);
    if (ALONE && zmask) atomicAdd(&n_zero, (uint32_t)__builtin_popcount(zmask));
    if (threadIdx.x == 0) node[1] = ALONE ? fe_inverse_binary(node[1], P) : fe_load(inv, blockIdx.x);
    Fe back = inv_tree_down(node, P);   // the inverse of x[0] ... x[kInvPerThread - 1]
    inv_static_for<0, kInvPerThread>([&](auto kc) {
        constexpr uint32_t q = kInvPerThread - 1 - decltype(kc)::value;
        const uint64_t i = base + (uint64_t)q * kBlock;
        const Fe o = q ? fe_mul_tt(back, pre[q], P) : back;
        if (q) back = fe_mul_tt(back, x[q], P);
        if (i < n) fe_store(out, i, (zmask >> q) & 1u ? fe_zero() : o);
    });
    if (ALONE && threadIdx.x == 0 && zero_count) *zero_count = n_zero;
}

// ---- running products: out[i] = t[0] ... t[i-1] (exclusive, out[0] = 1) or t[0] ... t[i] (INCLUSIVE).  Plain products: a zero
// propagates.  The order matters here, so thread t keeps a contiguous run of kPrefixPerThread elements (the layout of the
// interpolation's k_scan_prod_*: each lane strides 512 B; not this section's hot path).  Three launches.
constexpr uint32_t kPrefixPerThread = 16, kPrefixChunk = kBlock * kPrefixPerThread;
__global__ __launch_bounds__(kBlock) void k_prefix_partial(const uint64_t *__restrict__ v, uint64_t n, FieldParams P,
                                                           uint64_t *__restrict__ totals) {
    __shared__ Fe node[2 * kBlock];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPrefixChunk + (uint64_t)threadIdx.x * kPrefixPerThread;
    Fe acc = fe_one(P);
    for (uint32_t q = 0; q < kPrefixPerThread && i0 + q < n; ++q) acc = fe_mul_tt(acc, fe_load(v, i0 + q), P);
    inv_tree_up(acc, node, P);
    if (threadIdx.x == 0) fe_store(totals, blockIdx.x, node[1]);
}
// one workgroup: totals[0 .. nc) -> their exclusive prefixes, totals[nc] = the product of all
__global__ __launch_bounds__(kBlock) void k_prefix_totals(uint64_t *__restrict__ totals, uint64_t nc, FieldParams P) {
    __shared__ Fe red[kBlock];
    const uint64_t per = (nc + kBlock - 1) / kBlock, j0 = threadIdx.x * per, j1 = j0 + per < nc ? j0 + per : nc;
    Fe acc = fe_one(P);
    for (uint64_t j = j0; j < j1; ++j) acc = fe_mul_tt(acc, fe_load(totals, j), P);
    Fe total;
    Fe pre = block_scan_excl(acc, red, P, &total);
    for (uint64_t j = j0; j < j1; ++j) {
        const Fe x = fe_load(totals, j);
        fe_store(totals, j, pre);
        pre = fe_mul_tt(pre, x, P);
    }
    if (threadIdx.x == 0) fe_store(totals, nc, total);
}
// every element is read (twice) by the thread that writes it, before it writes it: out may be v (neither is __restrict__)
template <bool INCLUSIVE>
__global__ __launch_bounds__(kBlock) void k_prefix_apply(const uint64_t *v, uint64_t n, FieldParams P, const uint64_t *__restrict__ totals,
                                                         uint64_t *out) {
    __shared__ Fe red[kBlock];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPrefixChunk + (uint64_t)threadIdx.x * kPrefixPerThread;
    Fe acc = fe_one(P);
    for (uint32_t q = 0; q < kPrefixPerThread && i0 + q < n; ++q) acc = fe_mul_tt(acc, fe_load(v, i0 + q), P);
    Fe total;
    Fe pre = fe_mul_tt(fe_load(totals, blockIdx.x), block_scan_excl(acc, red, P, &total), P);
    for (uint32_t q = 0; q < kPrefixPerThread && i0 + q < n; ++q) {
        const Fe x = fe_load(v, i0 + q);
        if (INCLUSIVE) pre = fe_mul_tt(pre, x, P);
        fe_store(out, i0 + q, pre);
        if (!INCLUSIVE) pre = fe_mul_tt(pre, x, P);
    }
}

}  // namespace zk
