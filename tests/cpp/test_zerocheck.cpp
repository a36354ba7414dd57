// The zerocheck argument through the C++ host mirror (zk_amd/host/zk.hpp: Gate<F>::create, Zerocheck<F>::prove / verify / gate_sums /
// proof_bytes): proofs of x0 x1 - x2 = 0 that the host verifier accepts with the prover's own point and claims, the claims against the
// tables' evaluations, the verifier's verdicts after a changed seed, byte or table entry, gate_sums' first two sums against their
// check, the length formula and the error codes.  Built and run by tests/test_gpu_zerocheck.py (needs a gfx950 device to run).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;
using ZC = Zerocheck<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    try {
        const Fr one = Fr::from(1), minus_one = Fr::from_i64(-1), zero = Fr::from(0);
        Digest seed{};
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(11 * i + 3);
        Gate<F> gate = std::move(Gate<F>::create(3, {{one, {0, 1}}, {minus_one, {2}}}).unwrap());
        ASSERT(gate.degree() == 2 && gate.n_columns() == 3);
        for (const uint32_t n : {1u, 4u, 9u, 12u}) {
            const size_t len = (size_t)1 << n;
            std::vector<Fr> a(len), b(len), c(len);
            for (size_t i = 0; i < len; ++i) a[i] = Fr::from(i + 1), b[i] = Fr::from(2 * i + 3), c[i] = Fr::from((i + 1) * (2 * i + 3));
            const Mle ta = Mle::new_(n, a).unwrap(), tb = Mle::new_(n, b).unwrap(), tc = Mle::new_(n, c).unwrap();
            const std::vector<const Mle *> tabs = {&ta, &tb, &tc};
            ASSERT(ZC::proof_bytes(gate, n).unwrap() == 32ull * (3 * n + 3));
            const ZerocheckProof<F> pr = ZC::prove(tabs, gate, seed).unwrap();
            ASSERT(pr.proof.size() == 32ull * (3 * n + 3) && pr.point.size() == n && pr.claims.size() == 3);
            ASSERT(ZC::prove(tabs, gate, seed).unwrap().proof == pr.proof);   // the same bytes again
            const ZerocheckClaim<F> cl = ZC::verify(gate, n, seed, pr.proof).unwrap();
            ASSERT(cl.ok && cl.point == pr.point && cl.claims == pr.claims);
            ASSERT(ta.evaluate(pr.point).unwrap() == pr.claims[0] && tb.evaluate(pr.point).unwrap() == pr.claims[1] &&
                   tc.evaluate(pr.point).unwrap() == pr.claims[2]);
            for (size_t at : {(size_t)31, pr.proof.size() / 2, pr.proof.size() - 1}) {
                std::vector<uint8_t> bad = pr.proof;
                bad[at] ^= 0x04;
                ASSERT(!ZC::verify(gate, n, seed, bad).unwrap().ok);
            }
            if (n >= 2) {
                Digest other = seed;
                other[0] ^= 1;
                ASSERT(!ZC::verify(gate, n, other, pr.proof).unwrap().ok);
            }
            std::vector<uint8_t> cut(pr.proof.begin(), pr.proof.end() - 1);
            ASSERT(ZC::verify(gate, n, seed, cut).is_err());   // another length
            // a satisfied gate: g(0) = g(1) = 0 against any tail
            std::vector<Fr> tail(n - 1);
            for (size_t j = 0; j + 1 < n; ++j) tail[j] = Fr::from(5 * j + 2);
            const std::vector<Fr> sums = ZC::gate_sums(tabs, gate, tail).unwrap();
            ASSERT(sums.size() == 3 && sums[0] == zero && sums[1] == zero);
            // one violated row: the prover still makes a proof, and the verifier rejects it
            std::vector<Fr> c2 = c;
            c2[len / 3] = Fr::from(7);
            const Mle tc2 = Mle::new_(n, c2).unwrap();
            const ZerocheckProof<F> bad_pr = ZC::prove({&ta, &tb, &tc2}, gate, seed).unwrap();
            ASSERT(!ZC::verify(gate, n, seed, bad_pr.proof).unwrap().ok);
            ASSERT(ta.evaluation_slice() == a && tb.evaluation_slice() == b && tc.evaluation_slice() == c);   // left intact
        }
        ASSERT(ZC::proof_bytes(gate, 0).is_err() && ZC::proof_bytes(gate, 41).is_err());
        ASSERT(Gate<F>::create(3, {{one, {0, 3}}}).is_err() && Gate<F>::create(17, {{one, {0}}}).is_err() && Gate<F>::create(3, {{one, {}}}).is_err());
        const Mle small = Mle::new_(2, std::vector<Fr>(4, one)).unwrap(), big = Mle::new_(3, std::vector<Fr>(8, one)).unwrap();
        ASSERT(ZC::prove({&small, &small, &big}, gate, seed).is_err() && ZC::prove({&small, &small}, gate, seed).is_err());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: zerocheck host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
