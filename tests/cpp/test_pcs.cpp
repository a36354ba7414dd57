// The FRI polynomial commitment through the C++ host mirror (zk_amd/host/zk.hpp: Pcs<F>::commit / root / open / verify / proof_bytes /
// deep_quotient): openings whose values are the polynomials' evaluations and whose proofs the host verifier accepts, two openings of one
// commitment, the verifier's verdicts after a changed value, point, root, seed or byte, the length formula, the quotient of columns that
// equal their claimed values, and the error codes.  Built and run by tests/test_gpu_pcs.py (needs a gfx950 device to run).
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
        const uint32_t d = 9;
        std::vector<Poly> polys;
        for (uint64_t c = 0; c < 3; ++c) {
            std::vector<Fr> co(((size_t)1 << d) - c);   // 2^d, 2^d - 1, 2^d - 2 coefficients
            for (size_t i = 0; i < co.size(); ++i) co[i] = Fr::from((3 + c) * i * i + 7 * c + 1);
            polys.push_back(Poly::new_(co));
        }
        Digest seed{};
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(11 * i + 3);
        const FriParams shapes[] = {{9, 2, 3, 0, 8}, {9, 1, 2, 1, 8}, {9, 3, 1, 2, 1}};
        for (const FriParams &fp : shapes) {
            const Pcs<F> com = std::move(Pcs<F>::commit(polys, fp.log_degree, fp.log_blowup, fp.log_arity, five).unwrap());
            ASSERT(com.n_polys() == 3);
            const Digest root = com.root();
            const uint64_t want = Fri<F>::proof_bytes(fp).unwrap() +
                                  32ull * fp.n_queries * ((3ull << fp.log_arity) + fp.log_degree + fp.log_blowup - fp.log_arity);
            ASSERT(Pcs<F>::proof_bytes(3, fp).unwrap() == want);
            const Fr zs[2] = {Fr::from(123456789), zero};   // two openings of one commitment
            for (const Fr &z : zs) {
                const PcsOpening<F> o = com.open(z, fp.log_final, fp.n_queries, seed).unwrap();
                ASSERT(o.proof.size() == want && o.values.size() == 3);
                for (size_t c = 0; c < 3; ++c) ASSERT(o.values[c] == polys[c].evaluate(z));
                ASSERT(Pcs<F>::verify(root, z, o.values, o.proof, fp, five, seed).unwrap());
                ASSERT(com.open(z, fp.log_final, fp.n_queries, seed).unwrap().proof == o.proof);   // the same bytes again
                std::vector<Fr> other_values = o.values;
                other_values[1] = one;
                ASSERT(!Pcs<F>::verify(root, z, other_values, o.proof, fp, five, seed).unwrap());
                ASSERT(!Pcs<F>::verify(root, Fr::from(77), o.values, o.proof, fp, five, seed).unwrap());
                Digest other = root;
                other[5] ^= 2;
                ASSERT(!Pcs<F>::verify(other, z, o.values, o.proof, fp, five, seed).unwrap());
                other = seed;
                other[0] ^= 1;
                ASSERT(!Pcs<F>::verify(root, z, o.values, o.proof, fp, five, other).unwrap());
                for (size_t at : {(size_t)3, o.proof.size() / 2, o.proof.size() - 40, o.proof.size() - 1}) {
                    std::vector<uint8_t> bad = o.proof;
                    bad[at] ^= 0x04;
                    ASSERT(!Pcs<F>::verify(root, z, o.values, bad, fp, five, seed).unwrap());
                }
                std::vector<uint8_t> cut(o.proof.begin(), o.proof.end() - 1);
                ASSERT(Pcs<F>::verify(root, z, o.values, cut, fp, five, seed).is_err());   // another length
            }
            ASSERT(com.root() == root);   // the handle survives its openings
            ASSERT(com.open(five, fp.log_final, fp.n_queries, seed).is_err());                   // the shift itself is on the domain
            ASSERT(com.open(one, fp.log_final + fp.log_arity + 20, fp.n_queries, seed).is_err());   // log_final >= log_degree
            ASSERT(com.open(one, fp.log_final, 0, seed).is_err());
        }
        // columns that equal their claimed values everywhere: the numerator, and so the quotient, is zero whatever alpha and z are
        const std::vector<Fr> sevens((size_t)1 << 12, Fr::from(7)), nines((size_t)1 << 12, Fr::from(9)), zeros((size_t)1 << 12, zero);
        const std::vector<Mle> cols = {Mle::new_(12, sevens).unwrap(), Mle::new_(12, nines).unwrap()};
        ASSERT(Pcs<F>::deep_quotient(cols, five, Fr::from(3), {Fr::from(7), Fr::from(9)}, Fr::from(11)).unwrap().evaluation_slice() == zeros);
        ASSERT(cols[0].evaluation_slice() == sevens && cols[1].evaluation_slice() == nines);   // the columns are left intact
        ASSERT(Pcs<F>::deep_quotient(cols, five, five, {Fr::from(7), Fr::from(9)}, one).is_err());    // z on the domain
        ASSERT(Pcs<F>::deep_quotient(cols, zero, one, {Fr::from(7), Fr::from(9)}, one).is_err());     // the shift is zero
        ASSERT(Pcs<F>::deep_quotient(cols, five, one, {Fr::from(7)}, one).is_err());                  // a value per column
        // parameters that do not fit
        ASSERT(Pcs<F>::commit(polys, 8, 2, 3, five).is_err());    // 2^9 coefficients against a bound of 2^8
        ASSERT(Pcs<F>::commit(polys, 9, 0, 3, five).is_err() && Pcs<F>::commit(polys, 9, 2, 4, five).is_err() && Pcs<F>::commit(polys, 9, 2, 3, zero).is_err());
        ASSERT(Pcs<F>::commit({}, 9, 2, 3, five).is_err());
        ASSERT(Pcs<F>::commit(polys, 27, 2, 3, five).is_err());   // a domain past the two-adicity of BN254
        ASSERT(Pcs<F>::proof_bytes(129, {9, 2, 3, 0, 8}).is_err() && Pcs<F>::proof_bytes(3, {9, 2, 2, 0, 8}).is_err());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: pcs host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
