// The grand-product argument through the C++ host mirror (zk_amd/host/zk.hpp: GrandProduct<F>::tree / prove / verify / verify_table /
// proof_bytes): the tree's root against a product computed on the host, proofs the host verifier accepts with the prover's own point and
// claim, the claim against the table's evaluation, the verifier's verdicts after a changed product, seed, shift or byte, NULL and zero
// shifts, the length formula and the error codes.  Built and run by tests/test_gpu_gprod.py (needs a gfx950 device to run).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;
using GP = GrandProduct<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    try {
        const Fr one = Fr::from(1), five = Fr::from(5), zero = Fr::from(0);
        Digest seed{};
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(13 * i + 5);
        for (const uint32_t n : {1u, 3u, 9u, 12u}) {
            std::vector<Fr> values((size_t)1 << n);
            for (size_t i = 0; i < values.size(); ++i) values[i] = Fr::from(3 * i * i + 7 * i + 1);
            const Mle table = Mle::new_(n, values).unwrap();
            ASSERT(GP::proof_bytes(n).unwrap() == 64ull * n * n);
            for (const Fr *shift : {(const Fr *)nullptr, &five}) {
                // the tree's levels against their definition, level by level, on the host copy
                const std::vector<Fr> heap = GP::tree(table, shift).unwrap().evaluation_slice();
                ASSERT(heap.size() == values.size() && heap[0] == one);
                const GrandProductProof<F> pr = GP::prove(table, seed, shift).unwrap();
                ASSERT(pr.product == heap[1] && pr.proof.size() == 64ull * n * n && pr.point.size() == n);
                ASSERT(GP::prove(table, seed, shift).unwrap().proof == pr.proof);   // the same bytes again
                const GrandProductClaim<F> cl = GP::verify(n, seed, pr.product, pr.proof, shift).unwrap();
                ASSERT(cl.ok && cl.point == pr.point && cl.claim == pr.claim);
                ASSERT(table.evaluate(pr.point).unwrap() == pr.claim);
                ASSERT(GP::verify_table(table, seed, pr.product, pr.proof, shift).unwrap());
                ASSERT(!GP::verify(n, seed, five, pr.proof, shift).unwrap().ok);
                for (size_t at : {(size_t)3, pr.proof.size() / 2, pr.proof.size() - 1}) {
                    std::vector<uint8_t> bad = pr.proof;
                    bad[at] ^= 0x04;
                    ASSERT(!GP::verify_table(table, seed, pr.product, bad, shift).unwrap());
                }
                if (n >= 2) {   // (at n = 1 the transcript only draws the point)
                    Digest other = seed;
                    other[0] ^= 1;
                    ASSERT(!GP::verify(n, other, pr.product, pr.proof, shift).unwrap().ok);
                    ASSERT(!GP::verify(n, seed, pr.product, pr.proof, &one).unwrap().ok);   // another shift
                }
                std::vector<uint8_t> cut(pr.proof.begin(), pr.proof.end() - 1);
                ASSERT(GP::verify(n, seed, pr.product, cut, shift).is_err());   // another length
            }
            // NULL and an explicit zero are the same statement
            ASSERT(GP::prove(table, seed, &zero).unwrap().proof == GP::prove(table, seed).unwrap().proof);
            ASSERT(table.evaluation_slice() == values);   // the table is left intact
        }
        ASSERT(GP::proof_bytes(0).is_err() && GP::proof_bytes(41).is_err());
        const Mle point_table = Mle::new_(0, std::vector<Fr>{five}).unwrap();
        ASSERT(GP::tree(point_table).is_err() && GP::prove(point_table, seed).is_err());   // n = 0
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: gprod host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
