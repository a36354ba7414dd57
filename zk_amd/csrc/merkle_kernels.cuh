// merkle_kernels.cuh -- binary Keccak-256 Merkle commitments over one or more tables of field elements (no reference item; definition:
// tests/merkle_ref.py; host side merkle.hip; design DESIGN.md section 13).
//
//   leaf[i]        = Keccak256(be32(c_0[i]) || ... || be32(c_{k-1}[i]))      be32 = the 32-byte big-endian canonical integer (to_bytes)
//   level[d+1][j]  = Keccak256(level[d][2j] || level[d][2j+1]),  level[0] = leaf,  root = level[n][0]
//
// Every level is kept: the handle's one block holds level 0, then level 1, ... (merkle_level_offset), 2^(n+1) - 1 digests of 4 words.
// A permutation on one lane is several thousand VALU operations, so a commitment is bound by the ALU, not by the 32 bytes a digest moves:
// what the kernels have to get right is that the 25-word state never leaves the registers (no run-time index into it) and that the
// threads of a wave read consecutive elements of each column.  The statement digest of the GKR driver (gkr_kernels.cuh, 4-ary,
// 128-byte leaves) is another format and keeps its own kernels.
#pragma once
#include "common.cuh"
#include "transcript.cuh"

namespace zk {

constexpr uint32_t kMerkleMaxColumns = 1024;
constexpr uint32_t kMerkleMaxTileLog = 10;   // a tile of 2^10 digests is 32 KiB of LDS
constexpr uint32_t kMerkleTopLog = 6;        // at most 2^6 digests left: the top kernel's one workgroup finishes the tree
constexpr uint32_t kMerkleTopThreads = 1024; // 16 waves, one node each per step
constexpr uint32_t kMerklePtrBatch = 32;     // column pointers that one k_merkle_put_ptrs launch carries in its arguments

// first digest of level d in the handle's block, in digests: 2^n + 2^(n-1) + ... + 2^(n-d+1)
__host__ __device__ inline uint64_t merkle_level_offset(uint32_t n, uint32_t d) { return (2ull << n) - (2ull << (n - d)); }

struct MerklePtrs {
    const uint64_t *p[kMerklePtrBatch];
};
// The column pointers live in a device array (up to 1024 of them do not fit the kernel arguments of the hashing kernels); it is filled
// from the arguments of this launch, 32 at a time, so that a commitment stays stream-ordered without a host copy to wait for.
__global__ __launch_bounds__(64) void k_merkle_put_ptrs(const uint64_t **__restrict__ table, uint32_t base, uint32_t count, MerklePtrs b) {
    if (threadIdx.x < count) table[base + threadIdx.x] = b.p[threadIdx.x];
}

// Keccak256 of two digests (64 bytes: one block, the 0x01 of the padding in word 8, the 0x80 at the end of word 16)
ZK_D void merkle_node_hash(const uint64_t (&l)[4], const uint64_t (&r)[4], uint64_t (&out)[4]) {
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s[i] = l[i];
        s[4 + i] = r[i];
    }
    s[8] = 0x01ull;
#pragma unroll
    for (int i = 9; i < 25; ++i) s[i] = 0;
    s[16] = 0x8000000000000000ull;
    keccak_f1600(s);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = s[i];
}

// Keccak256 of row `row` of k columns.  The message is 4k words and the rate 17, so block b starts at word 17 b = 4 e0 + o with
// e0 = 17 b / 4 and o = b mod 4: it holds words o .. o + 16 of the five elements e0 .. e0 + 4.  Those twenty words sit in registers
// under compile-time names and the offset o is applied by masks, so no run-time index touches w[] or the state; the positions
// repeat every four blocks (17 elements).  The fifth element is the first one of the next block unless o = 3, so it is carried over
// instead of being loaded and converted twice.  Elements past k count as zero words, and the padding goes into the block that holds
// word 4k -- a block of its own when 4k is a multiple of 17 (k = 17, 34, ...).  The one permutation site keeps the code small.
ZK_D void merkle_leaf_hash(const uint64_t *const *__restrict__ cols, uint32_t k, uint64_t row, const FieldParams &P, uint64_t (&out)[4]) {
    uint64_t s[25], w[20];
#pragma unroll
    for (int i = 0; i < 25; ++i) s[i] = 0;
#pragma unroll
    for (int i = 0; i < 20; ++i) w[i] = 0;
    const uint32_t n_words = 4 * k, last = n_words / 17, pad_at = n_words - 17 * last;
#pragma unroll 1
    for (uint32_t blk = 0; blk <= last; ++blk) {
        const uint32_t o = blk & 3, e0 = (17 * blk) >> 2;
        const bool carried = blk != 0 && o != 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            if (i == 0 && carried) {
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = w[16 + j];
            } else if (e0 + i < k) {
                const Fe c = fe_to_canonical(fe_load(cols[e0 + i], row), P);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    w[4 * i + j] = WordSponge::bswap64((uint64_t)c.v[2 * (3 - j)] | ((uint64_t)c.v[2 * (3 - j) + 1] << 32));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) w[4 * i + j] = 0;
            }
        }
        // (masks, not selects between w[p + a] and w[p + b]: the compiler folds such a select into one load with a run-time index, which
        // sends w[] to scratch)
        const uint64_t m0 = o == 0 ? ~0ull : 0, m1 = o == 1 ? ~0ull : 0, m2 = o == 2 ? ~0ull : 0, m3 = o == 3 ? ~0ull : 0;
#pragma unroll
        for (int p = 0; p < 17; ++p) s[p] ^= (w[p] & m0) | (w[p + 1] & m1) | (w[p + 2] & m2) | (w[p + 3] & m3);
        if (blk == last) {
#pragma unroll
            for (int p = 0; p < 17; ++p)
                if ((uint32_t)p == pad_at) s[p] ^= 0x01ull;
            s[16] ^= 0x8000000000000000ull;
        }
        keccak_f1600(s);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = s[i];
}

ZK_D void merkle_load(const uint64_t *__restrict__ at, uint64_t (&d)[4]) {
    const uint4 a = reinterpret_cast<const uint4 *>(at)[0], b = reinterpret_cast<const uint4 *>(at)[1];
    d[0] = (uint64_t)a.x | ((uint64_t)a.y << 32), d[1] = (uint64_t)a.z | ((uint64_t)a.w << 32);
    d[2] = (uint64_t)b.x | ((uint64_t)b.y << 32), d[3] = (uint64_t)b.z | ((uint64_t)b.w << 32);
}
ZK_D void merkle_store(uint64_t *__restrict__ at, const uint64_t (&d)[4]) {
    reinterpret_cast<uint4 *>(at)[0] = make_uint4((uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32));
    reinterpret_cast<uint4 *>(at)[1] = make_uint4((uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32));
}

// ---- level by level: the simple form ----------------------------------------------------------------------------------------------
// level 0: one thread per row; a wave reads 64 consecutive elements of every column
__global__ __launch_bounds__(kBlock) void k_merkle_leaves(const uint64_t *const *__restrict__ cols, uint32_t k, uint64_t n_rows,
                                                          uint64_t *__restrict__ out, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_rows; i += stride) {
        uint64_t d[4];
        merkle_leaf_hash(cols, k, i, P, d);
        merkle_store(out + 4 * i, d);
    }
}
// one level: one thread per node
__global__ __launch_bounds__(kBlock) void k_merkle_level(const uint64_t *__restrict__ in, uint64_t n_out, uint64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n_out; j += stride) {
        uint64_t l[4], r[4], d[4];
        merkle_load(in + 8 * j, l);
        merkle_load(in + 8 * j + 4, r);
        merkle_node_hash(l, r, d);
        merkle_store(out + 4 * j, d);
    }
}
// One node on one wave with the lane-parallel permutation (transcript.cuh): `a` is the state word of this lane.
ZK_D uint64_t merkle_node_wave(uint64_t a, const LaneKeccak &L) {
    if (L.index == 8) a = 0x01ull;
    if (L.index == 16) a = 0x8000000000000000ull;
    return lane_keccak_f1600(a, L);
}
// the same level with one wave per node, for the small upper levels, which are pure latency (as k_tree_level_wave)
__global__ __launch_bounds__(64) void k_merkle_level_wave(const uint64_t *__restrict__ in, uint64_t *__restrict__ out) {
    const uint64_t j = blockIdx.x;
    const LaneKeccak L = lane_keccak_init();
    uint64_t a = 0;
    if (L.index >= 0 && L.index < 8) a = in[8 * j + (uint32_t)L.index];
    a = merkle_node_wave(a, L);
    if (L.index >= 0 && L.index < 4) out[4 * j + (uint32_t)L.index] = a;
}

// ---- fused sub-tree build -----------------------------------------------------------------------------------------------------------
// A workgroup takes a tile of 2^tile_log digests of level level_in -- LEAF: it hashes them from the columns (level_in = 0) -- and
// climbs tile_log levels with the digests in LDS, writing every level it produces to its place in `tree`.  A level is built in place:
// node j of a step reads slots 2j and 2j + 1 and lands in slot j after a barrier; a later step of the same level reads slots
// >= 2 (j0 + kBlock) > j0 + kBlock, which this step does not write.  Dynamic LDS: 32 bytes << tile_log.
template <bool LEAF>
__global__ __launch_bounds__(kBlock) void k_merkle_fused(const uint64_t *const *__restrict__ cols, uint32_t k, uint64_t *__restrict__ tree,
                                                         uint32_t n, uint32_t level_in, uint32_t tile_log, FieldParams P) {
    extern __shared__ uint64_t merkle_lds[];
    const uint32_t t = threadIdx.x, tile = 1u << tile_log;
    const uint64_t n_tiles = 1ull << (n - level_in - tile_log);
    for (uint64_t g = blockIdx.x; g < n_tiles; g += gridDim.x) {
        uint64_t *in = tree + 4 * (merkle_level_offset(n, level_in) + g * tile);
        for (uint32_t i = t; i < tile; i += kBlock) {
            uint64_t d[4];
            if (LEAF) {
                merkle_leaf_hash(cols, k, g * tile + i, P, d);
                merkle_store(in + 4 * i, d);
            } else {
                merkle_load(in + 4 * i, d);
            }
            merkle_store(merkle_lds + 4 * i, d);
        }
        __syncthreads();
        for (uint32_t d = 1; d <= tile_log; ++d) {
            const uint32_t m = tile >> d;
            uint64_t *out = tree + 4 * (merkle_level_offset(n, level_in + d) + g * m);
            for (uint32_t j0 = 0; j0 < m; j0 += kBlock) {
                const uint32_t j = j0 + t;
                uint64_t h[4];
                if (j < m) {
                    uint64_t l[4], r[4];
                    merkle_load(merkle_lds + 8 * j, l);
                    merkle_load(merkle_lds + 8 * j + 4, r);
                    merkle_node_hash(l, r, h);
                }
                __syncthreads();
                if (j < m) {
                    merkle_store(merkle_lds + 4 * j, h);
                    merkle_store(out + 4 * j, h);
                }
                __syncthreads();
            }
        }
    }
}
// The top of the tree in one workgroup: the 2^top_log <= 64 digests of level level_in to the root, one node per wave and step
// with the lane-parallel permutation (these levels are pure latency), built in place in LDS like the tiles above.
__global__ __launch_bounds__(kMerkleTopThreads) void k_merkle_top(uint64_t *__restrict__ tree, uint32_t n, uint32_t level_in, uint32_t top_log) {
    __shared__ uint64_t lds[4 << kMerkleTopLog];
    const uint32_t t = threadIdx.x, wave = t >> 6, n_waves = kMerkleTopThreads / 64;
    const LaneKeccak L = lane_keccak_init();
    const uint64_t *in = tree + 4 * merkle_level_offset(n, level_in);
    if (t < (4u << top_log)) lds[t] = in[t];
    __syncthreads();
    for (uint32_t d = 1; d <= top_log; ++d) {
        const uint32_t m = (1u << top_log) >> d;
        uint64_t *out = tree + 4 * merkle_level_offset(n, level_in + d);
        for (uint32_t j0 = 0; j0 < m; j0 += n_waves) {
            const uint32_t j = j0 + wave;   // wave-uniform
            uint64_t a = 0;
            if (j < m) {
                if (L.index >= 0 && L.index < 8) a = lds[8 * j + (uint32_t)L.index];
                a = merkle_node_wave(a, L);
            }
            __syncthreads();
            if (j < m && L.index >= 0 && L.index < 4) {
                lds[4 * j + (uint32_t)L.index] = a;
                out[4 * j + (uint32_t)L.index] = a;
            }
            __syncthreads();
        }
    }
}

// ---- openings ---------------------------------------------------------------------------------------------------------------------
// One launch for all queries.  Item (q, r): r < n copies the sibling digest level[r][(i_q >> r) ^ 1] to paths[q][r]; r >= n (only when
// cols != null: per = n + k) copies element i_q of column r - n to rows[q][r - n].  The host has checked every index < 2^n.
__global__ __launch_bounds__(kBlock) void k_merkle_gather(const uint64_t *__restrict__ tree, uint32_t n, const uint64_t *__restrict__ idx, uint64_t n_queries,
                                                          const uint64_t *const *__restrict__ cols, uint32_t k, uint64_t *__restrict__ paths,
                                                          uint64_t *__restrict__ rows) {
    const uint32_t per = n + (cols ? k : 0);
    const uint64_t total = n_queries * per, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < total; it += stride) {
        const uint64_t q = it / per, i = idx[q];
        const uint32_t r = (uint32_t)(it - q * per);
        uint64_t d[4];
        if (r < n) {
            merkle_load(tree + 4 * (merkle_level_offset(n, r) + ((i >> r) ^ 1)), d);
            merkle_store(paths + 4 * (q * n + r), d);
        } else {
            merkle_load(cols[r - n] + 4 * i, d);
            merkle_store(rows + 4 * (q * k + (r - n)), d);
        }
    }
}

}  // namespace zk
