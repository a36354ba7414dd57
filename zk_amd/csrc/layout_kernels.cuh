// layout_kernels.cuh -- sharding of a table by index mod W (the layout of zk_shard_prover_create and zk_ntt_sharded's strided
// input), and its inverse.  Pure permutations of 32-byte elements: no field arithmetic, bit-exact by construction.
//
//   split      : out[g][j] = in[j * W + g]      (one table of W * M elements -> W tables of M)
//   interleave : out[j * W + g] = in[g][j]      (W tables of M, or one rank-major [W][M] buffer -> one table)
//
// Read the natural table as a matrix of M rows j and W columns g: split is its transpose into W rows of M, interleave the
// transpose back.  Every access is 16 B per lane, two lanes per element (element e = uint4 slots 2e, 2e + 1), as in k_fold_msb.
//   * k_shard_split_direct / k_shard_interleave_direct (W <= 8, and any shape the tiles do not cover): the natural side moves
//     1 KiB runs per wave instruction, the shard side 1024 / W bytes per shard (>= 128 B for W <= 8).
//   * k_shard_split_tiled / k_shard_interleave_tiled (W >= kTileG, M >= kTileJ): a workgroup moves a tile of kTileJ rows x
//     kTileG columns through LDS.  The natural side reads / writes runs of kTileG elements (512 B) per row, the shard side
//     runs of kTileJ elements (1 KiB) per shard.  The LDS image is stored shard-major ([g][j], a row of 2 kTileJ slots plus
//     one element of padding): the shard side touches it in contiguous slots, and the natural side's 16 consecutive lanes
//     (one row j, 8 columns, both halves) fall on slot offsets 2 g + h (mod 16) -- 16 distinct 16-B bank groups.
// Shard addresses: `major` (one rank-major buffer, shard g at major + g * 2M slots), else ptrs.p[g] (W <= kShardArgPtrs,
// passed in the kernel arguments), or table[g] (a device pointer table the host stages for larger W).
// All indices are 64-bit: tables of up to 2^40 elements.
#pragma once
#include "common.cuh"

namespace zk {

constexpr int kShardArgPtrs = 64;
struct ShardPtrs {
    uint4 *p[kShardArgPtrs];
};
struct ShardSrc {   // where shard g lives (see above)
    uint4 *major;
    uint4 *const *table;
    ShardPtrs ptrs;
};
ZK_D uint4 *shard_base(const ShardSrc &s, uint64_t g, uint64_t m_slots) {
    if (s.major) return s.major + g * m_slots;
    return s.table ? s.table[g] : s.ptrs.p[g];
}

constexpr int kShardUnroll = 4;   // slots per lane in flight (a wave moves 4 KiB per iteration)
// ---- direct forms: lane l of a wave owns slots chunk * 256 + u * 64 + l, u < 4, of the natural table ----------------------
__global__ __launch_bounds__(kBlock) void k_shard_split_direct(const uint4 *__restrict__ in, ShardSrc out, uint32_t log_w, uint64_t n_slots) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint64_t m_slots = n_slots >> log_w, wmask = (1ull << log_w) - 1;
    for (uint64_t s0 = wave * 64 * kShardUnroll; s0 < n_slots; s0 += nwaves * 64 * kShardUnroll) {
        uint4 v[kShardUnroll];
#pragma unroll
        for (int u = 0; u < kShardUnroll; ++u) {
            const uint64_t s = s0 + u * 64 + lane;
            if (s < n_slots) v[u] = nt_load16(in + s);
        }
#pragma unroll
        for (int u = 0; u < kShardUnroll; ++u) {
            const uint64_t s = s0 + u * 64 + lane;
            if (s < n_slots) {
                const uint64_t e = s >> 1;
                nt_store16(v[u], shard_base(out, e & wmask, m_slots) + 2 * (e >> log_w) + (s & 1));
            }
        }
    }
}
__global__ __launch_bounds__(kBlock) void k_shard_interleave_direct(ShardSrc in, uint4 *__restrict__ out, uint32_t log_w, uint64_t n_slots) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint64_t m_slots = n_slots >> log_w, wmask = (1ull << log_w) - 1;
    for (uint64_t s0 = wave * 64 * kShardUnroll; s0 < n_slots; s0 += nwaves * 64 * kShardUnroll) {
        uint4 v[kShardUnroll];
#pragma unroll
        for (int u = 0; u < kShardUnroll; ++u) {
            const uint64_t s = s0 + u * 64 + lane;
            if (s < n_slots) {
                const uint64_t e = s >> 1;
                v[u] = nt_load16(shard_base(in, e & wmask, m_slots) + 2 * (e >> log_w) + (s & 1));
            }
        }
#pragma unroll
        for (int u = 0; u < kShardUnroll; ++u) {
            const uint64_t s = s0 + u * 64 + lane;
            if (s < n_slots) nt_store16(v[u], out + s);
        }
    }
}

// ---- tiled forms ---------------------------------------------------------------------------------------------------------
constexpr int kTileJ = 32, kTileG = 16;                      // rows (shard positions) x columns (shards) of one tile
constexpr int kTileSlots = 2 * kTileJ * kTileG;               // 1024 slots = 16 KiB
constexpr int kTileRowSlots = 2 * kTileJ + 2;                 // one shard's row in LDS, padded by one element
constexpr int kTilePerLane = kTileSlots / kBlock;             // 4
static_assert(kTileSlots % kBlock == 0, "tile must split evenly over the workgroup");
// q-th slot of the tile seen from the natural side (row r = q / 2G, column c = (q / 2) % G, half h) -> its LDS slot
ZK_D uint32_t tile_lds_natural(uint32_t q) {
    const uint32_t r = q / (2 * kTileG), cg = (q / 2) % kTileG, h = q & 1;
    return cg * kTileRowSlots + 2 * r + h;
}
// q-th slot seen from the shard side (column c = q / 2J, slots 2 r + h of its run) -> its LDS slot
ZK_D uint32_t tile_lds_shard(uint32_t q) { return (q / (2 * kTileJ)) * kTileRowSlots + q % (2 * kTileJ); }

// the natural table as M rows of W elements; tiles are numbered column block fastest (neighbouring workgroups read
// neighbouring 512-B pieces of the same rows)
__global__ __launch_bounds__(kBlock) void k_shard_split_tiled(const uint4 *__restrict__ in, ShardSrc out, uint32_t log_w, uint64_t m) {
    __shared__ uint4 tile[kTileG * kTileRowSlots];
    const uint64_t w = 1ull << log_w, gtiles = w / kTileG, ntiles = gtiles * (m / kTileJ);
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t g0 = (t % gtiles) * kTileG, j0 = (t / gtiles) * kTileJ;
        uint4 v[kTilePerLane];
#pragma unroll
        for (int u = 0; u < kTilePerLane; ++u) {
            const uint32_t q = u * kBlock + threadIdx.x;
            const uint32_t r = q / (2 * kTileG), c2 = q % (2 * kTileG);
            v[u] = nt_load16(in + 2 * ((j0 + r) * w + g0) + c2);
        }
#pragma unroll
        for (int u = 0; u < kTilePerLane; ++u) tile[tile_lds_natural(u * kBlock + threadIdx.x)] = v[u];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kTilePerLane; ++u) {
            const uint32_t q = u * kBlock + threadIdx.x;
            const uint32_t cg = q / (2 * kTileJ), r2 = q % (2 * kTileJ);
            nt_store16(tile[tile_lds_shard(q)], shard_base(out, g0 + cg, 2 * m) + 2 * j0 + r2);
        }
        __syncthreads();   // the next tile overwrites the LDS image
    }
}
__global__ __launch_bounds__(kBlock) void k_shard_interleave_tiled(ShardSrc in, uint4 *__restrict__ out, uint32_t log_w, uint64_t m) {
    __shared__ uint4 tile[kTileG * kTileRowSlots];
    const uint64_t w = 1ull << log_w, gtiles = w / kTileG, ntiles = gtiles * (m / kTileJ);
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t g0 = (t % gtiles) * kTileG, j0 = (t / gtiles) * kTileJ;
        uint4 v[kTilePerLane];
#pragma unroll
        for (int u = 0; u < kTilePerLane; ++u) {
            const uint32_t q = u * kBlock + threadIdx.x;
            const uint32_t cg = q / (2 * kTileJ), r2 = q % (2 * kTileJ);
            v[u] = nt_load16(shard_base(in, g0 + cg, 2 * m) + 2 * j0 + r2);
        }
#pragma unroll
        for (int u = 0; u < kTilePerLane; ++u) tile[tile_lds_shard(u * kBlock + threadIdx.x)] = v[u];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kTilePerLane; ++u) {
            const uint32_t q = u * kBlock + threadIdx.x;
            const uint32_t r = q / (2 * kTileG), c2 = q % (2 * kTileG);
            nt_store16(tile[tile_lds_natural(q)], out + 2 * ((j0 + r) * w + g0) + c2);
        }
        __syncthreads();
    }
}

}  // namespace zk
