// UnivariatePolynomial interpolation and Add through the C++ host mirror (zk_amd/host/zk.hpp): the reference's KATs
// (univariate_poly.rs:266-293, :322-350, :409-420), the repeated-x error, and one 2^20-point interpolate of a quadratic given as raw
// limbs (R^-1 c(i): the result's raw limbs are the quadratic's coefficients, then zeros).  Built and run by
// tests/test_gpu_upoly_interp.py and tests/test_upoly_interp_host.py (needs a gfx950 device to run).
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
        // test_polynomial_interpolation
        ASSERT(Poly::interpolate_xy(ints({0, 1}), ints({0, 2})).coefficients() == ints({0, 2}));
        ASSERT(Poly::interpolate_xy(ints({0, 1, 2}), ints({5, 7, 13})).coefficients() == ints({5, 0, 2}));
        ASSERT(Poly::interpolate_xy(ints({0, 1, 3, 4, 5, 8}), ints({12, 48, 3150, 11772, 33452, 315020})).coefficients() ==
               ints({12, 8, 1, 7, 12, 8}));   // the reference's [12, 25, 18, 24, 12, 8] mod 17
        const Poly p = Poly::interpolate_xy(ints({5, 7, 9, 1}), ints({565, 1631, 3537, -7}));
        ASSERT(p.coefficients() == ints({0, -12, 0, 5}));
        // test_univariate_polynomial_trait_methods
        const Poly zero = Poly::new_({});
        ASSERT((p + zero) == p);
        ASSERT(p.evaluate(Fr::from(5)) == Fr::from(565));
        // test_polynomial_addition
        ASSERT((zero + zero).len() == 0);
        ASSERT((zero + Poly::new_(ints({0, 2}))).coefficients() == ints({0, 2}));
        ASSERT((Poly::new_(ints({0, 2})) + zero).coefficients() == ints({0, 2}));
        const Poly a = Poly::new_(ints({4, 3, 2})), b = Poly::new_(ints({3, 4, 0, 4}));
        ASSERT((a + b) == (b + a));
        ASSERT((a + b).coefficients() == ints({7, 7, 2, 4}));
        // interpolate over 0 .. n-1 keeps n coefficients
        ASSERT(Poly::interpolate(ints({7, 7, 7})).coefficients() == ints({7, 0, 0}));
        // a repeated x: the reference panics, the mirror throws
        bool threw = false;
        try {
            (void)Poly::interpolate_xy(ints({3, 4, 3}), ints({1, 2, 3}));
        } catch (const std::runtime_error &) {
            threw = true;
        }
        ASSERT(threw);
        // 2^20 points of a raw-limb quadratic
        const uint64_t n = 1u << 20, a0 = 9876, a1 = 321, a2 = 17;
        std::vector<Fr> ys(n);
        for (uint64_t i = 0; i < n; ++i) ys[i].l = {a0 + a1 * i + a2 * i * i, 0, 0, 0};
        const std::vector<Fr> r = Poly::interpolate(ys).coefficients();
        ASSERT(r.size() == n);
        bool rest_zero = true;
        for (uint64_t i = 3; i < n; ++i) rest_zero = rest_zero && r[i].l == std::array<uint64_t, 4>{0, 0, 0, 0};
        ASSERT(r[0].l[0] == a0 && r[1].l[0] == a1 && r[2].l[0] == a2 && r[0].l[1] == 0 && r[2].l[3] == 0);
        ASSERT(rest_zero);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: upoly interpolation host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
