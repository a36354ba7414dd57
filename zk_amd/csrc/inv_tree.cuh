// inv_tree.cuh -- the workgroup's product tree in LDS behind Montgomery's trick, and the constant-index loop over a thread's register
// arrays: shared by the batch inversion (inv_kernels.cuh) and the DEEP quotient (pcs_kernels.cuh).  Device functions only, no kernel.
#pragma once
#include <type_traits>

#include "common.cuh"

namespace zk {

// Product tree over the block's kBlock thread values in LDS (2 * kBlock nodes): node[kBlock + t] = x of thread t,
// node[i] = node[2i] * node[2i + 1], node[1] = the product of all.  kBlock - 1 multiplications in all.
ZK_D void inv_tree_up(const Fe &x, Fe *node, const FieldParams &P) {
    const uint32_t t = threadIdx.x;
    node[kBlock + t] = x;
    __syncthreads();
    for (uint32_t w = kBlock / 2; w >= 1; w >>= 1) {
        if (t < w) node[w + t] = fe_mul_tt(node[2 * (w + t)], node[2 * (w + t) + 1], P);
        __syncthreads();
    }
}
// The way back: node[1] holds the INVERSE of the root (stored after inv_tree_up by one thread, no barrier needed in between); every
// node is replaced by its inverse, 1/left = 1/parent * right and 1/right = 1/parent * left.  Returns the inverse of thread t's value.
ZK_D Fe inv_tree_down(Fe *node, const FieldParams &P) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    for (uint32_t w = 1; w < kBlock; w <<= 1) {
        if (t < w) {
            const uint32_t i = w + t;
            const Fe inv = node[i], l = node[2 * i], r = node[2 * i + 1];
            node[2 * i] = fe_mul_tt(inv, r, P);
            node[2 * i + 1] = fe_mul_tt(inv, l, P);
        }
        __syncthreads();
    }
    return node[kBlock + t];
}
// f(integral_constant<I>) ... f(integral_constant<N - 1>): the per-thread loops index register arrays, so their indices must be
// constants whatever the unroller decides (a rolled loop puts the arrays into scratch)
template <uint32_t I, uint32_t N, class F>
ZK_D void inv_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<uint32_t, I>{});
        inv_static_for<I + 1, N>(f);
    }
}

}  // namespace zk
