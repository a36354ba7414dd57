// FRI low-degree proofs through the C++ host mirror (zk_amd/host/zk.hpp: Fri<F>::lde / fold / proof_bytes / prove / verify): the LDE of a
// constant, the fold of an LDE against the LDE of the folded coefficients (beta = 0 and beta = 1, where the folded coefficients are plain
// sums), proofs that the host verifier accepts, its verdicts after one flipped bit and under another seed, shift or parameter, the
// length formula and the error codes.  Built and run by tests/test_gpu_fri.py (needs a gfx950 device to run).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;
using Poly = UnivariatePolynomial<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    try {
        const Fr one = Fr::from(1), five = Fr::from(5), zero = Fr::from(0);
        // a constant polynomial evaluates to the constant everywhere; so does the empty one to zero
        const std::vector<Fr> sevens((size_t)1 << 6, Fr::from(7)), zeros((size_t)1 << 6, zero);
        ASSERT(Fri<F>::lde(Poly::new_({Fr::from(7)}), 6, five).unwrap().evaluation_slice() == sevens);
        ASSERT(Fri<F>::lde(Poly::new_({}), 6, five).unwrap().evaluation_slice() == zeros);
        ASSERT(Fri<F>::lde(Poly::new_(std::vector<Fr>(65, one)), 6, five).is_err());   // more than 2^log_n coefficients
        ASSERT(Fri<F>::lde(Poly::new_({one}), 6, zero).is_err());                       // the shift is zero
        // fold(lde(c)) = lde(c') on the shift^(2^a) coset, c'[m] = sum_j beta^j c[2^a m + j]: beta = 0 picks c[2^a m], beta = 1 the plain sums
        const uint32_t d = 9;
        std::vector<Fr> c((size_t)1 << d);
        for (size_t i = 0; i < c.size(); ++i) c[i] = Fr::from(3 * i * i + 1);
        const Poly p = Poly::new_(c);
        const Mle layer = Fri<F>::lde(p, d + 2, five).unwrap();
        uint64_t shift_pow = 5;
        for (uint32_t a = 1; a <= 3; ++a) {
            shift_pow *= shift_pow;   // 5^(2^a)
            std::vector<Fr> picked(c.size() >> a), summed(c.size() >> a);
            for (size_t m = 0; m < picked.size(); ++m) {
                uint64_t s = 0;
                for (size_t j = 0; j < ((size_t)1 << a); ++j) s += 3 * ((m << a) + j) * ((m << a) + j) + 1;
                picked[m] = c[m << a];
                summed[m] = Fr::from(s);
            }
            const Fr s_a = Fr::from(shift_pow);
            ASSERT(Fri<F>::fold(layer, a, five, zero).unwrap().evaluation_slice() == Fri<F>::lde(Poly::new_(picked), d + 2 - a, s_a).unwrap().evaluation_slice());
            ASSERT(Fri<F>::fold(layer, a, five, one).unwrap().evaluation_slice() == Fri<F>::lde(Poly::new_(summed), d + 2 - a, s_a).unwrap().evaluation_slice());
        }
        ASSERT(layer.evaluation_slice() == Fri<F>::lde(p, d + 2, five).unwrap().evaluation_slice());   // the input is left intact
        ASSERT(Fri<F>::fold(layer, 0, five, one).is_err() && Fri<F>::fold(layer, 4, five, one).is_err());
        ASSERT(Fri<F>::fold(layer, 1, zero, one).is_err());
        ASSERT(Fri<F>::fold(Mle::new_(1, {one, five}).unwrap(), 2, five, one).is_err());              // fewer variables than the arity
        // proofs
        Digest seed{};
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(7 * i + 1);
        const FriParams shapes[] = {{9, 2, 3, 0, 8}, {9, 1, 2, 1, 8}, {9, 3, 1, 2, 1}};
        for (const FriParams &fp : shapes) {
            const uint32_t rounds = (fp.log_degree - fp.log_final) / fp.log_arity;
            uint64_t per_query = 0;
            for (uint32_t r = 0; r < rounds; ++r) per_query += ((uint64_t)1 << fp.log_arity) + fp.log_degree + fp.log_blowup - fp.log_arity * (r + 1);
            const uint64_t want = 32 * (rounds + ((uint64_t)1 << fp.log_final) + fp.n_queries * per_query);
            ASSERT(Fri<F>::proof_bytes(fp).unwrap() == want);
            const std::vector<uint8_t> proof = Fri<F>::prove(p, fp, five, seed).unwrap();
            ASSERT(proof.size() == want);
            ASSERT(Fri<F>::verify(proof, fp, five, seed).unwrap());
            ASSERT(Fri<F>::prove(p, fp, five, seed).unwrap() == proof);   // the same bytes again
            for (size_t at : {(size_t)3, (size_t)32 * rounds + 31, proof.size() / 2, proof.size() - 1}) {
                std::vector<uint8_t> bad = proof;
                bad[at] ^= 0x04;
                ASSERT(!Fri<F>::verify(bad, fp, five, seed).unwrap());
            }
            Digest other = seed;
            other[0] ^= 1;
            ASSERT(!Fri<F>::verify(proof, fp, five, other).unwrap());
            ASSERT(!Fri<F>::verify(proof, fp, one, seed).unwrap());
            FriParams more = fp;
            more.n_queries += 1;
            ASSERT(Fri<F>::verify(proof, more, five, seed).is_err());   // another length
            std::vector<uint8_t> cut(proof.begin(), proof.end() - 1);
            ASSERT(Fri<F>::verify(cut, fp, five, seed).is_err());
        }
        // one coefficient over the bound, and parameters that do not fit
        ASSERT(Fri<F>::prove(Poly::new_(std::vector<Fr>(((size_t)1 << 9) + 1, one)), shapes[0], five, seed).is_err());
        ASSERT(Fri<F>::prove(p, {9, 2, 2, 0, 8}, five, seed).is_err());    // 2 does not divide 9
        ASSERT(Fri<F>::prove(p, {9, 2, 3, 9, 8}, five, seed).is_err());    // log_final >= log_degree
        ASSERT(Fri<F>::prove(p, {9, 0, 3, 0, 8}, five, seed).is_err() && Fri<F>::prove(p, {9, 2, 3, 0, 0}, five, seed).is_err());
        ASSERT(Fri<F>::prove(p, {27, 2, 3, 0, 8}, five, seed).is_err());   // a domain past the two-adicity of BN254
        ASSERT(Fri<F>::proof_bytes({9, 2, 4, 1, 8}).is_err());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: fri host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
