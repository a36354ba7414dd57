// Division with remainder and the series inverse through the C++ host mirror (zk_amd/host/zk.hpp: divrem, operator/, operator%,
// inverse_series): cases by hand, the length conventions (nothing trimmed, la < lb, lb = 1), the zero leading coefficient, and one
// 2^12 round trip by construction -- a = q0 b + r0 formed with the product and the sum, divrem(a, b) must return (q0, r0).  Built
// and run by tests/test_gpu_upoly_divrem.py (needs a gfx950 device to run).
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Poly = UnivariatePolynomial<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static std::vector<Fr> ints(std::initializer_list<int64_t> v) {
    std::vector<Fr> c;
    for (int64_t x : v) c.push_back(Fr::from_i64(x));
    return c;
}

int main() {
    try {
        // x^3 + 2x^2 + 3x + 4 = (x^2 + x + 2)(x + 1) + 2
        const Poly a = Poly::new_(ints({4, 3, 2, 1})), b = Poly::new_(ints({1, 1}));
        auto qr = a.divrem(b);
        ASSERT(qr.first.coefficients() == ints({2, 1, 1}));
        ASSERT(qr.second.coefficients() == ints({2}));
        ASSERT((a / b).coefficients() == ints({2, 1, 1}));
        ASSERT((a % b).coefficients() == ints({2}));
        // nothing is trimmed: a zero-topped dividend keeps its length in q, and r is always lb - 1 long
        qr = Poly::new_(ints({4, 3, 2, 1, 0, 0})).divrem(Poly::new_(ints({0, 0, 1})));
        ASSERT(qr.first.coefficients() == ints({2, 1, 0, 0}));
        ASSERT(qr.second.coefficients() == ints({4, 3}));
        qr = Poly::new_(ints({7, 8})).divrem(Poly::new_(ints({1, 2, 3})));   // la < lb
        ASSERT(qr.first.len() == 0 && qr.second.coefficients() == ints({7, 8}));
        qr = Poly::new_(ints({6, 8, 10})).divrem(Poly::new_(ints({2})));     // lb = 1
        ASSERT(qr.first.coefficients() == ints({3, 4, 5}) && qr.second.len() == 0);
        qr = a.divrem(a);                                                    // a == b
        ASSERT(qr.first.coefficients() == ints({1}) && qr.second.coefficients() == ints({0, 0, 0}));
        bool threw = false;
        try {
            (void)a.divrem(Poly::new_(ints({1, 0})));   // the leading coefficient is inverted
        } catch (const std::exception &) {
            threw = true;
        }
        ASSERT(threw);
        // 1 / (1 - x) = 1 + x + x^2 + ..
        ASSERT(Poly::new_(ints({1, -1})).inverse_series(5).coefficients() == ints({1, 1, 1, 1, 1}));
        ASSERT(Poly::new_(ints({1, -1})).inverse_series(0).len() == 0);
        // 2^12: Newton with an NTT product, by construction
        const uint64_t k = (1u << 12) - 200, lb = 201;
        std::vector<Fr> q0(k), bv(lb), r0(lb - 1);
        for (uint64_t i = 0; i < k; ++i) q0[i] = Fr::from(i * i + 3);
        for (uint64_t i = 0; i < lb; ++i) bv[i] = Fr::from(5 * i + 1);
        for (uint64_t i = 0; i + 1 < lb; ++i) r0[i] = Fr::from(11 * i + 7);
        const Poly pb = Poly::new_(bv), big = Poly::new_(q0) * pb + Poly::new_(r0);
        ASSERT(big.len() == (1u << 12));
        qr = big.divrem(pb);
        ASSERT(qr.first.coefficients() == q0);
        ASSERT(qr.second.coefficients() == r0);
        const Poly g = pb.inverse_series(300);
        std::vector<Fr> back = (pb * g).coefficients();
        back.resize(300);
        std::vector<Fr> one(300, Fr::from(0));
        one[0] = Fr::from(1);
        ASSERT(back == one);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: upoly divrem host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
