// UnivariatePolynomial::evaluate at many points through the C++ host mirror (zk_amd/host/zk.hpp, evaluate_many): a small case by
// hand, the empty polynomial and the empty point vector, and one 2^12 case -- the polynomial through 2^12 distinct points,
// evaluated back at them, must return the ys, and agree with evaluate() at a few of them.  Built and run by
// tests/test_gpu_upoly_evalmany.py (needs a gfx950 device to run).
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
        const Poly q = Poly::new_(ints({1, 2, 3}));   // 1 + 2x + 3x^2
        ASSERT(q.evaluate_many(ints({0, 1, 2, -1, 2})) == ints({1, 6, 17, 2, 17}));
        ASSERT(q.evaluate_many(Poly::new_({})).len() == 0);
        ASSERT(Poly::new_({}).evaluate_many(ints({4, 5})) == ints({0, 0}));
        ASSERT(q.evaluate_many(q).coefficients() == ints({6, 17, 34}));   // p == xs
        const uint64_t n = 1u << 12;
        std::vector<Fr> xs(n), ys(n);
        for (uint64_t i = 0; i < n; ++i) {
            xs[i] = Fr::from(7 * i + 3);
            ys[i] = Fr::from(i * i + 5);
        }
        const Poly p = Poly::interpolate_xy(xs, ys), xv = Poly::new_(xs);
        ASSERT(p.len() == n);
        const Poly back = p.evaluate_many(xv);
        ASSERT(back.len() == n);
        const std::vector<Fr> got = back.coefficients();
        ASSERT(got == ys);
        for (uint64_t i = 0; i < n; i += 293) ASSERT(p.evaluate(xs[i]) == got[i]);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: upoly evaluate_many host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
