// perm_kernels.cuh -- gfx950 kernels of the wiring (copy-constraint) permutation argument (no reference item; definition:
// tests/perm_ref.py; host side: perm.hip).
//
// The fingerprint table F of N = n + kappa + 1 variables over k witness columns w_c and k permutation columns sigma_c of n variables each
// (K = 2^kappa >= k): for the cell v = c 2^n + i, F[2v] = w_c[i] + beta v + gamma and F[2v + 1] = w_c[i] + beta sigma_c[i] + gamma; the
// padding columns c >= k hold ones.  The side bit is the index's lowest, so the product tree (gprod_kernels.cuh: the top index bit goes
// first) ends in the pair (identity side's product, sigma side's product).
//
// k_perm_leaves writes F, one cell per thread: the default route, the tree's launches follow (perm.hip).  k_perm_tree<A> (ZK_PERM_FUSE=1,
// which measures slower: profiles/perm.log) is k_ptree<A> with the leaves made in registers: the w columns and the
// sigma columns are each ONE virtual column of K 2^n elements (column = v >> n, row = v & (2^n - 1)); a lane owns the cells e + s M,
// s < 2^A, M = 2^(N - A - 1) -- the 2^A streams of k_ptree<A> over each virtual column -- reads w and sigma there, makes the label beta v
// with one multiplication and 2^A - 1 additions, writes both sides' leaves as one 64-byte pair per cell (level N, which the top layer's
// sumcheck reads) and multiplies A levels down on both sides into the heap.  F is never read back by the tree's first launch, and a
// padding column costs no load.  N - A >= 10 (the tree's LDS stage takes over there) and kappa <= 4, so n >= 6 there: a wave's run of
// 64 cells lies in one column.
#pragma once
#include "common.cuh"

namespace zk {

constexpr uint32_t kPermMaxCols = 16;
// levels k_perm_tree takes per launch: 2^2 cells of two sides are 8 elements in registers, as many as k_ptree<3> holds; with three levels
// (16 elements) the compiler spills (profiles/perm_resource_usage.md), so that instantiation is not shipped
constexpr uint32_t kPermMaxFuse = 2;

struct PermCols {   // the 2 k column pointers as a kernel argument: w_0 .. w_{k-1}, sigma_0 .. sigma_{k-1}
    const uint64_t *p[2 * kPermMaxCols];
};
struct PermArgs {
    const uint64_t *const *cols;   // the same 2 k pointers in device memory
    uint32_t n, k;
    Fe gamma, one;
    Fe beta_rr;       // beta R^2 mod p: an index v as a raw integer times it is the Montgomery form of beta v
    Fe beta_stride;   // beta M (k_perm_tree: the label's step from stream s to s + 1)
    Mul29 beta29;     // beta as a prepared multiplier
};

// the pointer table of a launch, from the kernel arguments to device memory (every index a constant: scalar loads, vector stores)
__global__ __launch_bounds__(64) void k_perm_cols(PermCols cols, const uint64_t **__restrict__ out) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 2 * (int)kPermMaxCols; ++i) out[i] = cols.p[i];
    }
}

ZK_D Fe perm_index(uint64_t v) {
    Fe r = {{(uint32_t)v, (uint32_t)(v >> 32), 0, 0, 0, 0, 0, 0}};
    return r;
}
// one cell's pair of leaves as 64 contiguous bytes
ZK_D void perm_pair_store(uint64_t *base, uint64_t v, const Fe &a, const Fe &b) {
    fe_store(base, 2 * v, a);
    fe_store(base, 2 * v + 1, b);
}
ZK_D void perm_pair_store_nt(uint64_t *base, uint64_t v, const Fe &a, const Fe &b) {
    uint4 *q = reinterpret_cast<uint4 *>(base + 8 * v);
    nt_store16(make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]), q);
    nt_store16(make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]), q + 1);
    nt_store16(make_uint4(b.v[0], b.v[1], b.v[2], b.v[3]), q + 2);
    nt_store16(make_uint4(b.v[4], b.v[5], b.v[6], b.v[7]), q + 3);
}

// F[2v], F[2v + 1] for every cell v < cells = K 2^n, one cell per thread on a grid-stride loop
__global__ __launch_bounds__(kBlock) void k_perm_leaves(PermArgs a, uint64_t cells, uint64_t *__restrict__ F, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, mask = (1ull << a.n) - 1;
    for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < cells; v += stride) {
        const uint32_t col = (uint32_t)(v >> a.n);
        if (col >= a.k) {
            perm_pair_store(F, v, a.one, a.one);
            continue;
        }
        const uint64_t row = v & mask;
        const Fe base = fe_add(fe_load(a.cols[col], row), a.gamma, P);
        const Fe id = fe_add(base, fe_mul(perm_index(v), a.beta_rr, P), P);
        const Fe sg = fe_add(base, fe_mul29(fe_load(a.cols[a.k + col], row), a.beta29, P), P);
        perm_pair_store(F, v, id, sg);
    }
}

// xi[s], xs[s] <- the products of the cells s and s + 2^L on each side, stored as pairs at level m + 1 + L of the heap (m = log2 M
// cells: level m + 1 + L has 2^(L+1) M entries, entry 2 (e + s M) + side), down to L = 0
template <int L>
ZK_D void perm_levels(Fe *xi, Fe *xs, uint64_t *__restrict__ heap, uint32_t m, uint64_t e, const FieldParams &P) {
    const uint64_t M = 1ull << m;
#pragma unroll
    for (int s = 0; s < (1 << L); ++s) {
        xi[s] = fe_mul_tt(xi[s], xi[s + (1 << L)], P);
        xs[s] = fe_mul_tt(xs[s], xs[s + (1 << L)], P);
        uint64_t *lvl = heap + 4 * ((2 * M) << L);
        if (L == 0) perm_pair_store(lvl, e + (uint64_t)s * M, xi[s], xs[s]);   // the next launch reads it
        else perm_pair_store_nt(lvl, e + (uint64_t)s * M, xi[s], xs[s]);       // read again only by the layer's sumcheck
    }
    if constexpr (L > 0) perm_levels<L - 1>(xi, xs, heap, m, e, P);
}
// Level N = m + 1 + A (F, written here) -> levels N - 1 .. N - A of the heap.  M = 2^m cells per stream, a multiple of 64; 2^n a multiple
// of 64 too.  The grid may be capped: a wave loops over runs of 64 cells.
template <int A>
__global__ __launch_bounds__(kBlock) void k_perm_tree(PermArgs a, uint32_t m, uint64_t *__restrict__ F, uint64_t *__restrict__ heap, FieldParams P) {
    static_assert(A >= 1 && A <= (int)kPermMaxFuse, "the instantiations without scratch");
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t M = 1ull << m, mask = (1ull << a.n) - 1;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t e0 = wave * 64; e0 < M; e0 += nwaves * 64) {
        const uint64_t e = e0 + pair_owned(lane);   // the cell of stream 0 this lane owns after run_load
        Fe xi[1 << A], xs[1 << A];
        Fe label = fe_mul(perm_index(e), a.beta_rr, P);
#pragma unroll
        for (int s = 0; s < (1 << A); ++s) {
            const uint64_t v0 = e0 + (uint64_t)s * M;   // wave-uniform: the run's first cell
            const uint32_t col = __builtin_amdgcn_readfirstlane((uint32_t)(v0 >> a.n));
            if (col < a.k) {
                const uint64_t row0 = v0 & mask;
                const Fe base = fe_add(run_load_nt(a.cols[col] + 4 * row0, lane), a.gamma, P);
                xi[s] = fe_add(base, label, P);
                xs[s] = fe_add(base, fe_mul29(run_load_nt(a.cols[a.k + col] + 4 * row0, lane), a.beta29, P), P);
            } else {
                xi[s] = a.one;
                xs[s] = a.one;
            }
            perm_pair_store_nt(F, e + (uint64_t)s * M, xi[s], xs[s]);
            if (s + 1 < (1 << A)) label = fe_add(label, a.beta_stride, P);
        }
        perm_levels<A - 1>(xi, xs, heap, m, e, P);
    }
}

}  // namespace zk
