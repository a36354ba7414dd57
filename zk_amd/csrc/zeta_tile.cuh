// zeta_tile.cuh -- the 64-KiB LDS tile shared by the zeta passes (zeta_kernels.cuh) and the dense coefficient transforms
// (cmle_kernels.cuh): its size, its swizzle and the butterfly levels inside it.  Layout notes: zeta_kernels.cuh.
#pragma once
#include "common.cuh"

namespace zk {

constexpr uint32_t kZetaTileLog = 11;
constexpr uint32_t kZetaTile = 1u << kZetaTileLog;                 // entries per tile: 64 KiB
constexpr uint32_t kZetaPlaneBytes = kZetaTile * 16 + 64;          // the high plane starts 64 B off a 128-B boundary: the lane pairs of the
                                                                   // HBM -> LDS transfer (low half, high half of one entry) write distinct banks
constexpr uint32_t kZetaLdsBytes = 2 * kZetaPlaneBytes;            // 131,200 B for two workgroups: two per CU

ZK_D uint32_t zeta_slot(uint32_t i) { return i ^ ((i >> 3) & 15u); }

// the G levels of bits [s, s + G) of the tile-local index, for every entry of a tile of 2^tile_log entries
template <int G>
ZK_D void zeta_group(unsigned char *smem, uint32_t s, uint32_t tile_log, const FieldParams &P) {
    uint4 *plo = reinterpret_cast<uint4 *>(smem), *phi = reinterpret_cast<uint4 *>(smem + kZetaPlaneBytes);
    const uint32_t items = 1u << (tile_log - G);
    for (uint32_t w = threadIdx.x; w < items; w += kBlock) {
        const uint32_t low = w & ((1u << s) - 1u), high = w >> s;
        const uint32_t i0 = (high << (s + G)) | low;
        Fe x[1 << G];
#pragma unroll
        for (int u = 0; u < (1 << G); ++u) {
            const uint32_t sl = zeta_slot(i0 | ((uint32_t)u << s));
            const uint4 a = plo[sl], b = phi[sl];
            x[u] = {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
        }
#pragma unroll
        for (int b = 0; b < G; ++b)
#pragma unroll
            for (int c = 0; c < (1 << G); ++c)
                if (c & (1 << b)) x[c] = fe_add(x[c], x[c ^ (1 << b)], P);
#pragma unroll
        for (int u = 1; u < (1 << G); ++u) {   // entry 0 of a group never changes
            const uint32_t sl = zeta_slot(i0 | ((uint32_t)u << s));
            plo[sl] = make_uint4(x[u].v[0], x[u].v[1], x[u].v[2], x[u].v[3]);
            phi[sl] = make_uint4(x[u].v[4], x[u].v[5], x[u].v[6], x[u].v[7]);
        }
    }
}
// levels of bits [lb, lb + L) of the tile-local index; ends with the tile complete in LDS (barrier included)
ZK_D void zeta_levels(unsigned char *smem, uint32_t lb, uint32_t L, uint32_t tile_log, const FieldParams &P) {
    for (uint32_t s = lb; s < lb + L;) {
        const uint32_t g = lb + L - s >= 3 ? 3u : lb + L - s;
        __syncthreads();
        if (g == 3) zeta_group<3>(smem, s, tile_log, P);
        else if (g == 2) zeta_group<2>(smem, s, tile_log, P);
        else zeta_group<1>(smem, s, tile_log, P);
        s += g;
    }
    __syncthreads();
}

}  // namespace zk
