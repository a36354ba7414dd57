// The multilinear polynomial commitment through the C++ host mirror (zk_amd/host/zk.hpp: MlPcs<F>::commit / root / open / verify /
// proof_bytes / eq_sums): openings whose value is the table's evaluation and whose proofs the host verifier accepts, several openings of
// one commitment, the verifier's verdicts after a changed value, point, root, seed or byte, the length formula, the two sums of a round
// against the evaluation they add up to, and the error codes.  Built and run by tests/test_gpu_mlpcs.py (needs a gfx950 device to run).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    try {
        const Fr one = Fr::from(1), five = Fr::from(5), zero = Fr::from(0);
        const uint32_t n = 11;
        std::vector<Fr> values((size_t)1 << n);
        for (size_t i = 0; i < values.size(); ++i) values[i] = Fr::from(3 * i * i + 7 * i + 1);
        const Mle table = Mle::new_(n, values).unwrap();
        Digest seed{};
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(11 * i + 3);
        std::vector<Fr> z1(n), z2(n);
        for (uint32_t j = 0; j < n; ++j) z1[j] = Fr::from(1000003ull * j + 17), z2[j] = j % 3 == 0 ? zero : j % 3 == 1 ? one : Fr::from_i64(-1);
        struct Shape {
            uint32_t b, f, q;
        };
        const Shape shapes[] = {{1, 0, 8}, {2, 3, 8}, {3, 1, 1}};
        for (const Shape &sh : shapes) {
            const MlPcs<F> com = std::move(MlPcs<F>::commit(table, sh.b, five).unwrap());
            ASSERT(com.n_vars() == n);
            const Digest root = com.root();
            const uint32_t R = n - sh.f;
            uint64_t want = 32ull * (3 * R + R - 1 + (1ull << sh.f));
            for (uint32_t r = 0; r < R; ++r) want += 32ull * sh.q * (2 + n + sh.b - 1 - r);
            ASSERT(MlPcs<F>::proof_bytes(n, sh.b, sh.f, sh.q).unwrap() == want);
            for (const std::vector<Fr> *z : {&z1, &z2, &z1}) {   // several openings of one commitment
                const MlPcsOpening<F> o = com.open(*z, sh.f, sh.q, seed).unwrap();
                ASSERT(o.proof.size() == want);
                ASSERT(o.value == table.evaluate(*z).unwrap());
                ASSERT(MlPcs<F>::verify(root, *z, o.value, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                ASSERT(com.open(*z, sh.f, sh.q, seed).unwrap().proof == o.proof);   // the same bytes again
                ASSERT(!MlPcs<F>::verify(root, *z, one, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                std::vector<Fr> other_point = *z;
                other_point[n - 1] = Fr::from(77);
                ASSERT(!MlPcs<F>::verify(root, other_point, o.value, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                Digest other = root;
                other[5] ^= 2;
                ASSERT(!MlPcs<F>::verify(other, *z, o.value, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                other = seed;
                other[0] ^= 1;
                ASSERT(!MlPcs<F>::verify(root, *z, o.value, o.proof, sh.b, sh.f, sh.q, five, other).unwrap());
                ASSERT(!MlPcs<F>::verify(root, *z, o.value, o.proof, sh.b, sh.f, sh.q, one, seed).unwrap());   // another shift
                for (size_t at : {(size_t)3, o.proof.size() / 2, o.proof.size() - 40, o.proof.size() - 1}) {
                    std::vector<uint8_t> bad = o.proof;
                    bad[at] ^= 0x04;
                    ASSERT(!MlPcs<F>::verify(root, *z, o.value, bad, sh.b, sh.f, sh.q, five, seed).unwrap());
                }
                std::vector<uint8_t> cut(o.proof.begin(), o.proof.end() - 1);
                ASSERT(MlPcs<F>::verify(root, *z, o.value, cut, sh.b, sh.f, sh.q, five, seed).is_err());   // another length
            }
            ASSERT(com.root() == root);   // the handle survives its openings
            ASSERT(com.open(z1, n, sh.q, seed).is_err());   // log_final >= n_vars
            ASSERT(com.open(z1, sh.f, 0, seed).is_err());
            ASSERT(com.open(std::vector<Fr>(n - 1, one), sh.f, sh.q, seed).is_err());   // a point of another arity
        }
        ASSERT(table.evaluation_slice() == values);   // the table is left intact
        // the two sums of a round are the evaluations at z_0 = 0 and z_0 = 1: t(z) = (1 - z_0) S_0 + z_0 S_1
        for (const std::vector<Fr> *z : {&z1, &z2}) {
            const std::array<Fr, 2> s = MlPcs<F>::eq_sums(table, std::vector<Fr>(z->begin() + 1, z->end())).unwrap();
            std::vector<Fr> at0 = *z, at1 = *z;
            at0[0] = zero, at1[0] = one;
            ASSERT(s[0] == table.evaluate(at0).unwrap() && s[1] == table.evaluate(at1).unwrap());
        }
        ASSERT(MlPcs<F>::eq_sums(table, z1).is_err());   // a tail has n_vars - 1 elements
        // parameters that do not fit
        ASSERT(MlPcs<F>::commit(table, 0, five).is_err() && MlPcs<F>::commit(table, 9, five).is_err() && MlPcs<F>::commit(table, 2, zero).is_err());
        ASSERT(MlPcs<F>::proof_bytes(0, 1, 0, 8).is_err() && MlPcs<F>::proof_bytes(4, 1, 4, 8).is_err() && MlPcs<F>::proof_bytes(4, 1, 0, 1025).is_err());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: mlpcs host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
