// Device harness for the field primitives (zk_amd/csrc/field.cuh and the lazy [0, 2p) helpers of ntt_kernels.cuh): reads a
// binary case file, runs ONE plain grid-stride kernel per primitive over it (one case per thread) and writes the raw output
// limbs to a file.  It holds no expectations: every expected value comes from Python integers (tests/field_corpus.py,
// driven by tests/test_gpu_field_device.py).  Standalone: it does not link libzk_amd.so.
//
// Built twice from this source with hipcc --offload-arch=gfx950: as shipped (the v_mad_u64_u32 / v_addc_co_u32 chains of
// mac, mac_col<N>, mac_col_s<N>, mac_s, acc_add32) and with -DZK_NO_ASM (the plain C++ bodies), so that a mismatch can be
// laid at the door of the asm chain or of the algorithm.  A third build with plain clang++ (-x c++, no HIP) runs the same
// cases through the host compilation of field.cuh in a CPU loop: tests/test_field_corpus_host.py checks the Python model
// against it before a GPU sees the corpus (the lazy helpers are device-only and are left out of that build).
//
// Case file (all u32, little endian): magic, field, number of sections; then per section a header
//   op, param, mode, n_a, n_b
// and its data.  mode 0: n_a cases of in_words(op, param) words each (n_b = 0).  mode 1 (two-operand primitives only): n_a
// elements A then n_b elements B of 8 words each; case i is (A[i / n_b], B[i % n_b]) -- the full cross product without
// writing it out.  Output file: for every section in order, out_words(op) words per case.
//
//   usage: test_field_device <cases.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#include "../../zk_amd/csrc/ntt_kernels.cuh"   // fe_add2, fe_sub2, fe_canon2, Mod2p (pulls in field.cuh)
#endif
#include "../../zk_amd/csrc/host_field.hpp"    // FieldParams tables (field_info)

using namespace zk;

enum Op : uint32_t {
    OP_ADD = 0, OP_SUB, OP_NEG, OP_MUL, OP_SQR, OP_MULWIDE_REDC, OP_WIDE, OP_MUL29, OP_MUL29_LAZY, OP_MUL_TT, OP_DOT2,
    OP_ADD2, OP_SUB2, OP_CANON2, OP_REDUCE_U256, OP_FROM_CANONICAL, OP_TO_CANONICAL, OP_FROM_U32, OP_PREPARE, OP_COUNT
};
constexpr uint32_t kMagic = 0x46454431u;   // "1DEF"

ZK_HD uint32_t in_words(uint32_t op, uint32_t param) {
    switch (op) {
    case OP_NEG: case OP_SQR: case OP_CANON2: case OP_REDUCE_U256: case OP_FROM_CANONICAL: case OP_TO_CANONICAL: case OP_PREPARE: return 8;
    case OP_FROM_U32: return 1;
    case OP_DOT2: return 32;
    case OP_WIDE: return 16 * param;   // param = N products: a_0, b_0, a_1, b_1, ...
    default: return 16;
    }
}
ZK_HD uint32_t out_words(uint32_t op) {
    switch (op) {
    case OP_MULWIDE_REDC: return 24;   // the 512-bit product, then its reduction
    case OP_WIDE: return 25;           // the 17-limb running sum, then its reduction
    case OP_PREPARE: return 9;         // nine 29-bit limbs
    default: return 8;
    }
}

ZK_HD Fe load_fe(const uint32_t *w) {
    Fe r;
    for (int i = 0; i < 8; ++i) r.v[i] = w[i];
    return r;
}
ZK_HD void store_fe(uint32_t *w, const Fe &r) {
    for (int i = 0; i < 8; ++i) w[i] = r.v[i];
}

// one case of primitive OP: `a` and `b` point at the case's operands (b = a + 8 in mode 0), `out` at its out_words(OP) words
template <uint32_t OP>
ZK_HD void run_case(const uint32_t *a, const uint32_t *b, uint32_t param, uint32_t *out, const FieldParams &P) {
    if constexpr (OP == OP_ADD) store_fe(out, fe_add(load_fe(a), load_fe(b), P));
    else if constexpr (OP == OP_SUB) store_fe(out, fe_sub(load_fe(a), load_fe(b), P));
    else if constexpr (OP == OP_NEG) store_fe(out, fe_neg(load_fe(a), P));
    else if constexpr (OP == OP_MUL) store_fe(out, fe_mul(load_fe(a), load_fe(b), P));
    else if constexpr (OP == OP_SQR) store_fe(out, fe_sqr(load_fe(a), P));
    else if constexpr (OP == OP_MULWIDE_REDC) {
        const Fe x = load_fe(a), y = load_fe(b);
        uint32_t t[16];
        mul_wide(t, x.v, y.v);
        for (int i = 0; i < 16; ++i) out[i] = t[i];
        store_fe(out + 16, redc(t, P));
    } else if constexpr (OP == OP_WIDE) {
        WideAcc w;
        wide_zero(w);
        for (uint32_t i = 0; i < param; ++i) {
            const Fe x = load_fe(a + 16 * i), y = load_fe(a + 16 * i + 8);
            wide_mac(w, x.v, y.v);
        }
        for (int i = 0; i < 17; ++i) out[i] = w.v[i];
        store_fe(out + 17, redc_wide(w, P));
    } else if constexpr (OP == OP_MUL29) store_fe(out, fe_mul29(load_fe(a), mul29_prepare(load_fe(b), P), P));
    else if constexpr (OP == OP_MUL29_LAZY) store_fe(out, fe_mul29_t<true>(load_fe(a), mul29_prepare(load_fe(b), P), P));
    else if constexpr (OP == OP_MUL_TT) store_fe(out, fe_mul_tt(load_fe(a), load_fe(b), P));
    else if constexpr (OP == OP_DOT2)
        store_fe(out, fe_dot2_29(load_fe(a), mul29_prepare(load_fe(a + 8), P), load_fe(a + 16), mul29_prepare(load_fe(a + 24), P), P));
#if defined(__HIPCC__)
    else if constexpr (OP == OP_ADD2) store_fe(out, fe_add2(load_fe(a), load_fe(b), mod2p_of(P)));
    else if constexpr (OP == OP_SUB2) store_fe(out, fe_sub2(load_fe(a), load_fe(b), mod2p_of(P)));
    else if constexpr (OP == OP_CANON2) store_fe(out, fe_canon2(load_fe(a), P));
#endif
    else if constexpr (OP == OP_REDUCE_U256) store_fe(out, fe_reduce_u256(a, P));
    else if constexpr (OP == OP_FROM_CANONICAL) store_fe(out, fe_from_canonical(load_fe(a), P));
    else if constexpr (OP == OP_TO_CANONICAL) store_fe(out, fe_to_canonical(load_fe(a), P));
    else if constexpr (OP == OP_FROM_U32) store_fe(out, fe_from_u32(a[0], P));
    else if constexpr (OP == OP_PREPARE) {
        const Mul29 m = mul29_prepare(load_fe(a), P);
        for (int i = 0; i < 9; ++i) out[i] = m.l[i];
    }
}

struct Section {
    uint32_t op, param, mode, n_a, n_b;
    uint64_t n_cases, in_off, out_off;   // word offsets into the case data / the output
};

// case i of a section: operand pointers
ZK_HD void case_operands(const Section &s, const uint32_t *in, uint64_t i, const uint32_t *&a, const uint32_t *&b) {
    if (s.mode == 1) {
        a = in + s.in_off + 8 * (i / s.n_b);
        b = in + s.in_off + 8 * ((uint64_t)s.n_a + i % s.n_b);
    } else {
        a = in + s.in_off + (uint64_t)in_words(s.op, s.param) * i;
        b = a + 8;
    }
}

#if defined(__HIPCC__)
template <uint32_t OP>
__global__ void __launch_bounds__(256) k_run(Section s, const uint32_t *in, uint32_t *out, FieldParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s.n_cases; i += stride) {
        const uint32_t *a, *b;
        case_operands(s, in, i, a, b);
        run_case<OP>(a, b, s.param, out + s.out_off + (uint64_t)out_words(OP) * i, P);
    }
}
#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
            return 3;                                                                              \
        }                                                                                          \
    } while (0)
#endif

template <uint32_t OP>
static int run_section(const Section &s, const uint32_t *in, uint32_t *out, const FieldParams &P) {
#if defined(__HIPCC__)
    const uint64_t blocks = (s.n_cases + 255) / 256;
    k_run<OP><<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256)>>>(s, in, out, P);
    CHECK(hipGetLastError());
#else
    if (OP == OP_ADD2 || OP == OP_SUB2 || OP == OP_CANON2) {
        fprintf(stderr, "op %u is device-only\n", OP);
        return 2;
    }
    for (uint64_t i = 0; i < s.n_cases; ++i) {
        const uint32_t *a, *b;
        case_operands(s, in, i, a, b);
        run_case<OP>(a, b, s.param, out + s.out_off + (uint64_t)out_words(OP) * i, P);
    }
#endif
    return 0;
}
template <uint32_t OP = 0>
static int dispatch(const Section &s, const uint32_t *in, uint32_t *out, const FieldParams &P) {
    if (s.op == OP) return run_section<OP>(s, in, out, P);
    if constexpr (OP + 1 < OP_COUNT) return dispatch<OP + 1>(s, in, out, P);
    return 2;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <cases.bin> <out.bin>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 12 || bytes % 4) { fprintf(stderr, "%s: bad size\n", argv[1]); return 2; }
    std::vector<uint32_t> file((size_t)bytes / 4);
    if (fread(file.data(), 4, file.size(), f) != file.size()) { fprintf(stderr, "%s: short read\n", argv[1]); return 2; }
    fclose(f);
    if (file[0] != kMagic) { fprintf(stderr, "%s: bad magic\n", argv[1]); return 2; }
    const FieldInfo *fi = field_info((int)file[1]);
    if (!fi) { fprintf(stderr, "unknown field %u\n", file[1]); return 2; }
    // parse and bounds-check every section before anything runs
    std::vector<Section> secs;
    uint64_t pos = 3, out_total = 0;
    for (uint32_t k = 0; k < file[2]; ++k) {
        if (pos + 5 > file.size()) { fprintf(stderr, "section %u: truncated header\n", k); return 2; }
        Section s = {file[pos], file[pos + 1], file[pos + 2], file[pos + 3], file[pos + 4], 0, pos + 5, out_total};
        if (s.op >= OP_COUNT || s.mode > 1 || (s.op == OP_WIDE && (s.param < 1 || s.param > (uint32_t)kMaxLazy))) {
            fprintf(stderr, "section %u: bad op / mode / param\n", k);
            return 2;
        }
        uint64_t words;
        if (s.mode == 1) {
            if (in_words(s.op, s.param) != 16 || s.n_b == 0) { fprintf(stderr, "section %u: cross product needs two operands\n", k); return 2; }
            s.n_cases = (uint64_t)s.n_a * s.n_b;
            words = 8ull * ((uint64_t)s.n_a + s.n_b);
        } else {
            s.n_cases = s.n_a;
            words = (uint64_t)in_words(s.op, s.param) * s.n_a;
        }
        if (pos + 5 + words > file.size()) { fprintf(stderr, "section %u: truncated data\n", k); return 2; }
        pos += 5 + words;
        out_total += s.n_cases * out_words(s.op);
        secs.push_back(s);
    }
    std::vector<uint32_t> out((size_t)out_total);
#if defined(__HIPCC__)
    uint32_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, file.size() * 4));
    CHECK(hipMalloc(&d_out, (out_total ? out_total : 1) * 4));
    CHECK(hipMemcpy(d_in, file.data(), file.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xA5, (out_total ? out_total : 1) * 4));
    for (const Section &s : secs)
        if (int rc = dispatch(s, d_in, d_out, fi->P)) return rc;
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out_total * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
#else
    for (const Section &s : secs)
        if (int rc = dispatch(s, file.data(), out.data(), fi->P)) return rc;
#endif
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), 4, out.size(), g) != out.size()) { fprintf(stderr, "%s: short write\n", argv[2]); return 2; }
    fclose(g);
    printf("ok: field %u, %zu sections, %llu output words\n", file[1], secs.size(), (unsigned long long)out_total);
    return 0;
}
