// The fractional-sum argument and the lookup multiplicities through the C++ host mirror (zk_amd/host/zk.hpp: FractionalSum<F>::tree / prove /
// verify / proof_bytes / multiplicities, lookup_multiplicities): the Q heap against GrandProduct's tree, the roots against the proof's sum,
// proofs the host verifier accepts with the prover's own point and claims, the claims against the tables' evaluations, the verifier's
// verdicts after a changed sum, seed, shift, has_p or byte, NULL and zero shifts, a zero denominator, the multiplicities of a small lookup,
// the length formula and the error codes.  Built and run by tests/test_gpu_fsum.py (needs a gfx950 device to run).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;
using FS = FractionalSum<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    try {
        const Fr one = Fr::from(1), five = Fr::from(5), zero = Fr::from(0);
        Digest seed{};
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(11 * i + 3);
        for (const uint32_t n : {1u, 3u, 9u, 12u}) {
            std::vector<Fr> qv((size_t)1 << n), pv((size_t)1 << n);
            for (size_t i = 0; i < qv.size(); ++i) qv[i] = Fr::from(3 * i * i + 7 * i + 1), pv[i] = Fr::from(i * i + 2);
            const Mle q = Mle::new_(n, qv).unwrap(), p = Mle::new_(n, pv).unwrap();
            ASSERT(FS::proof_bytes(n).unwrap() == 64ull * n * (n + 1));
            for (const Mle *pp : {(const Mle *)nullptr, &p}) {
                for (const Fr *shift : {(const Fr *)nullptr, &five}) {
                    const FractionTree<F> heaps = FS::tree(pp, q, shift).unwrap();
                    const std::vector<Fr> hp = heaps.p.evaluation_slice(), hq = heaps.q.evaluation_slice();
                    ASSERT(hp.size() == qv.size() && hp[0] == zero && hq[0] == one);
                    ASSERT(hq == GrandProduct<F>::tree(q, shift).unwrap().evaluation_slice());   // the Q heap is the product tree
                    const FractionalSumProof<F> pr = FS::prove(pp, q, seed, shift).unwrap();
                    ASSERT(pr.numerator == hp[1] && pr.denominator == hq[1] && pr.proof.size() == 64ull * n * (n + 1) && pr.point.size() == n);
                    ASSERT(FS::prove(pp, q, seed, shift).unwrap().proof == pr.proof);   // the same bytes again
                    const FractionalSumClaim<F> cl = FS::verify(n, pp != nullptr, seed, pr.numerator, pr.denominator, pr.proof, shift).unwrap();
                    ASSERT(cl.ok && cl.point == pr.point && cl.p_claim == pr.p_claim && cl.q_claim == pr.q_claim);
                    ASSERT(q.evaluate(pr.point).unwrap() == pr.q_claim);
                    ASSERT(pp ? p.evaluate(pr.point).unwrap() == pr.p_claim : pr.p_claim == one);
                    ASSERT(!FS::verify(n, pp != nullptr, seed, five, pr.denominator, pr.proof, shift).unwrap().ok);
                    ASSERT(!FS::verify(n, pp != nullptr, seed, pr.numerator, five, pr.proof, shift).unwrap().ok);
                    ASSERT(!FS::verify(n, pp != nullptr, seed, pr.numerator, zero, pr.proof, shift).unwrap().ok);   // D = 0
                    if (pp) ASSERT(!FS::verify(n, false, seed, pr.numerator, pr.denominator, pr.proof, shift).unwrap().ok);   // another has_p
                    for (size_t at : {(size_t)3, pr.proof.size() / 2, pr.proof.size() - 1}) {
                        std::vector<uint8_t> bad = pr.proof;
                        bad[at] ^= 0x04;
                        const FractionalSumClaim<F> b = FS::verify(n, pp != nullptr, seed, pr.numerator, pr.denominator, bad, shift).unwrap();
                        ASSERT(!b.ok || !(q.evaluate(b.point).unwrap() == b.q_claim) || (pp && !(p.evaluate(b.point).unwrap() == b.p_claim)));
                    }
                    if (n >= 2) {   // (at n = 1 the transcript only draws the point)
                        Digest other = seed;
                        other[0] ^= 1;
                        ASSERT(!FS::verify(n, pp != nullptr, other, pr.numerator, pr.denominator, pr.proof, shift).unwrap().ok);
                        ASSERT(!FS::verify(n, pp != nullptr, seed, pr.numerator, pr.denominator, pr.proof, &one).unwrap().ok);   // another shift
                    }
                    std::vector<uint8_t> cut(pr.proof.begin(), pr.proof.end() - 1);
                    ASSERT(FS::verify(n, pp != nullptr, seed, pr.numerator, pr.denominator, cut, shift).is_err());   // another length
                }
                // NULL and an explicit zero are the same statement
                ASSERT(FS::prove(pp, q, seed, &zero).unwrap().proof == FS::prove(pp, q, seed).unwrap().proof);
            }
            ASSERT(q.evaluation_slice() == qv && p.evaluation_slice() == pv);   // the tables are left intact
        }
        {   // a zero denominator: q[2] + shift = 0 is proven with D = 0, which the verifier rejects
            std::vector<Fr> qv(8);
            for (size_t i = 0; i < 8; ++i) qv[i] = Fr::from(i + 1);
            const Mle q = Mle::new_(3, qv).unwrap();
            const Fr minus3 = Fr::from_i64(-3);
            const FractionalSumProof<F> pr = FS::prove(nullptr, q, seed, &minus3).unwrap();
            ASSERT(pr.denominator == zero);
            ASSERT(!FS::verify(3, false, seed, pr.numerator, pr.denominator, pr.proof, &minus3).unwrap().ok);
        }
        {   // a small lookup: rows 10, 20, 30, 20 (a duplicate); the witness holds 10 five times, 20 twice, 30 never, and one 99
            const std::vector<Fr> tv = {Fr::from(10), Fr::from(20), Fr::from(30), Fr::from(20)};
            const std::vector<Fr> wv = {Fr::from(10), Fr::from(20), Fr::from(10), Fr::from(99), Fr::from(20), Fr::from(10), Fr::from(10), Fr::from(10)};
            const Mle t = Mle::new_(2, tv).unwrap(), w = Mle::new_(3, wv).unwrap();
            const LookupMultiplicities<F> lm = lookup_multiplicities(t, w).unwrap();
            const std::vector<Fr> want = {Fr::from(5), Fr::from(2), zero, zero};
            ASSERT(lm.m.evaluation_slice() == want && lm.missing == 1 && lm.first_missing == 3 && lm.duplicates == 1);
            const LookupMultiplicities<F> self = lookup_multiplicities(t, t).unwrap();
            const std::vector<Fr> want_self = {one, Fr::from(2), one, zero};
            ASSERT(self.m.evaluation_slice() == want_self && self.missing == 0 && self.first_missing == ~0ull && self.duplicates == 1);
            ASSERT(t.evaluation_slice() == tv && w.evaluation_slice() == wv);
        }
        ASSERT(FS::proof_bytes(0).is_err() && FS::proof_bytes(41).is_err());
        const Mle point_table = Mle::new_(0, std::vector<Fr>{five}).unwrap();
        ASSERT(FS::tree(nullptr, point_table).is_err() && FS::prove(nullptr, point_table, seed).is_err());   // n = 0
        const Mle two = Mle::new_(1, std::vector<Fr>{five, one}).unwrap(), four = Mle::new_(2, std::vector<Fr>{five, one, one, one}).unwrap();
        ASSERT(FS::tree(&two, four).is_err() && FS::prove(&two, four, seed).is_err());   // p and q of different sizes
        ASSERT(lookup_multiplicities(point_table, point_table).unwrap().missing == 0);   // n = 0 is a table of one row
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: fsum host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
