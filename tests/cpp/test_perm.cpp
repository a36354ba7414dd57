// The wiring (copy-constraint) permutation argument through the C++ host mirror (zk_amd/host/zk.hpp: Permutation<F>::fingerprint / prove /
// verify / proof_bytes, GrandProduct<F>::tree): two columns whose cells are wired in pairs across the columns; proofs that the host verifier accepts with the
// prover's own point and claims, the claims against the columns' evaluations, the fingerprint table's two side products, the verifier's
// verdicts after a changed seed, challenge, byte or witness entry, the length formula and the error codes.  Built and run by
// tests/test_gpu_perm.py (needs a gfx950 device to run).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;
using PM = Permutation<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    try {
        const uint64_t beta_v = 0x1234567, gamma_v = 0x89abcd;
        const Fr beta = Fr::from(beta_v), gamma = Fr::from(gamma_v);
        Digest seed{};
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(7 * i + 5);
        for (const uint32_t n : {1u, 4u, 9u, 11u}) {
            const size_t len = (size_t)1 << n;
            // cell (0, i) and cell (1, len - 1 - i) hold one value and are wired to each other
            std::vector<Fr> w0(len), w1(len), s0(len), s1(len);
            for (size_t i = 0; i < len; ++i) {
                w0[i] = Fr::from(3 * i + 1), w1[len - 1 - i] = w0[i];
                s0[i] = Fr::from(len + (len - 1 - i)), s1[len - 1 - i] = Fr::from(i);
            }
            const Mle t0 = Mle::new_(n, w0).unwrap(), t1 = Mle::new_(n, w1).unwrap(), u0 = Mle::new_(n, s0).unwrap(), u1 = Mle::new_(n, s1).unwrap();
            const PM::Columns w = {&t0, &t1}, sg = {&u0, &u1};
            const uint64_t N = n + 2, want = 32ull * (2 * N * N + 4);
            ASSERT(PM::proof_bytes(n, 2).unwrap() == want);
            const PermutationProof<F> pr = PM::prove(w, sg, beta, gamma, seed).unwrap();
            ASSERT(pr.proof.size() == want && pr.point.size() == n && pr.claims.size() == 4);
            ASSERT(PM::prove(w, sg, beta, gamma, seed).unwrap().proof == pr.proof);   // the same bytes again
            const PermutationClaim<F> cl = PM::verify(n, 2, beta, gamma, seed, pr.proof).unwrap();
            ASSERT(cl.ok && cl.point == pr.point && cl.claims == pr.claims);
            ASSERT(t0.evaluate(pr.point).unwrap() == pr.claims[0] && t1.evaluate(pr.point).unwrap() == pr.claims[1] &&
                   u0.evaluate(pr.point).unwrap() == pr.claims[2] && u1.evaluate(pr.point).unwrap() == pr.claims[3]);
            // the fingerprint table: 2^N entries, the first and the last cell's pairs by hand (the values are small integers), and the two
            // side products -- level 1 of its product tree -- equal
            const Mle fp = PM::fingerprint(w, sg, beta, gamma).unwrap();
            const std::vector<Fr> f = fp.evaluation_slice();
            ASSERT(f.size() == ((size_t)1 << N));
            ASSERT(f[0] == Fr::from(1 + gamma_v) && f[1] == Fr::from(1 + beta_v * (2 * len - 1) + gamma_v));
            ASSERT(f[4 * len - 2] == Fr::from(1 + beta_v * (2 * len - 1) + gamma_v) && f[4 * len - 1] == Fr::from(1 + gamma_v));
            const std::vector<Fr> heap = GrandProduct<F>::tree(fp).unwrap().evaluation_slice();
            ASSERT(heap[2] == heap[3]);
            for (size_t at : {(size_t)31, pr.proof.size() / 2, pr.proof.size() - 1}) {
                std::vector<uint8_t> bad = pr.proof;
                bad[at] ^= 0x04;
                ASSERT(!PM::verify(n, 2, beta, gamma, seed, bad).unwrap().ok);
            }
            Digest other = seed;
            other[0] ^= 1;
            ASSERT(!PM::verify(n, 2, beta, gamma, other, pr.proof).unwrap().ok);
            ASSERT(!PM::verify(n, 2, gamma, beta, seed, pr.proof).unwrap().ok);
            std::vector<uint8_t> cut(pr.proof.begin(), pr.proof.end() - 1);
            ASSERT(PM::verify(n, 2, beta, gamma, seed, cut).is_err());   // another length
            // one broken copy: the prover still makes a proof, and the verifier rejects it
            std::vector<Fr> w1b = w1;
            w1b[len / 3] = Fr::from(99999999);
            const Mle t1b = Mle::new_(n, w1b).unwrap();
            const PermutationProof<F> bad_pr = PM::prove({&t0, &t1b}, sg, beta, gamma, seed).unwrap();
            ASSERT(!PM::verify(n, 2, beta, gamma, seed, bad_pr.proof).unwrap().ok);
            ASSERT(t0.evaluation_slice() == w0 && t1.evaluation_slice() == w1 && u0.evaluation_slice() == s0 && u1.evaluation_slice() == s1);
        }
        ASSERT(PM::proof_bytes(0, 1).is_err() && PM::proof_bytes(4, 0).is_err() && PM::proof_bytes(4, 17).is_err() && PM::proof_bytes(40, 1).is_err());
        ASSERT(PM::proof_bytes(38, 1).unwrap() == 32ull * (2 * 39 * 39 + 2) && PM::proof_bytes(35, 16).unwrap() == 32ull * (2 * 40 * 40 + 32));
        const Mle small = Mle::new_(2, std::vector<Fr>(4, beta)).unwrap(), big = Mle::new_(3, std::vector<Fr>(8, beta)).unwrap();
        ASSERT(PM::prove({&small, &big}, {&small, &small}, beta, gamma, seed).is_err() && PM::prove({&small}, {&small, &small}, beta, gamma, seed).is_err());
        ASSERT(PM::prove({&small, nullptr}, {&small, &small}, beta, gamma, seed).is_err());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: permutation host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
