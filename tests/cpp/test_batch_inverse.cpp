// Batch inversion and running products through the C++ host mirror (zk_amd/host/zk.hpp: batch_inverse, batch_inverse_in_place,
// prefix_product, prefix_product_in_place, zk::batch_inverse): inverses known by hand, x * (1 / x) = 1 over 2^13 elements through
// ProductPoly::prod_reduce, zeros and their count, a zero that only the shift makes, in place against out of place, every vector
// length's handle, and the running products of small tables by hand.  Built and run by tests/test_gpu_batch_inverse.py (needs a
// gfx950 device to run).
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Poly = UnivariatePolynomial<F>;
using Mle = MultiLinearPolynomial<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static std::vector<Fr> ints(std::initializer_list<int64_t> v) {
    std::vector<Fr> c;
    for (int64_t x : v) c.push_back(Fr::from_i64(x));
    return c;
}

int main() {
    try {
        // 1 / 1 = 1, 1 / -1 = -1, 0 stays 0; 1 / (1 / x) = x
        uint64_t zeros = 99;
        const Poly v = Poly::new_(ints({1, -1, 0, 7, 0}));
        const Poly inv = v.batch_inverse(nullptr, &zeros);
        ASSERT(zeros == 2 && inv.len() == 5);
        const std::vector<Fr> iv = inv.coefficients();
        ASSERT(iv[0] == Fr::from(1) && iv[1] == Fr::from_i64(-1) && iv[2] == Fr::from(0) && iv[4] == Fr::from(0));
        ASSERT(inv.batch_inverse().coefficients() == v.coefficients());
        ASSERT(Poly::new_({}).batch_inverse(nullptr, &zeros).len() == 0 && zeros == 0);
        // a zero that only the shift makes: 1 / (x + 3) at x = -3, -2, -4
        const Fr three = Fr::from(3);
        const std::vector<Fr> sh = Poly::new_(ints({-3, -2, -4})).batch_inverse(&three, &zeros).coefficients();
        ASSERT(zeros == 1 && sh == ints({0, 1, -1}));
        ASSERT(batch_inverse<F>(ints({-3, -2, -4}), &three, &zeros) == ints({0, 1, -1}) && zeros == 1);
        ASSERT(batch_inverse<F>({}).empty());
        // 2^13 elements (four chunks): t * (1 / t) = 1 except at the planted zeros, in and out of place
        const size_t n_vars = 13, n = (size_t)1 << n_vars;
        std::vector<Fr> t(n);
        for (size_t i = 0; i < n; ++i) t[i] = Fr::from(i * i + 5 * i + 1);
        t[0] = t[2047] = t[2048] = t[n - 1] = Fr::from(0);
        Mle mt = Mle::new_(n_vars, t).unwrap();
        Mle mi = mt.batch_inverse(nullptr, &zeros).unwrap();
        ASSERT(zeros == 4);
        ASSERT(mt.evaluation_slice() == t);
        const std::vector<Fr> prod = ProductPoly<F>::new_({mt, mi}).unwrap().prod_reduce();
        size_t wrong = 0;
        for (size_t i = 0; i < n; ++i) wrong += prod[i] != Fr::from(i == 0 || i == 2047 || i == 2048 || i == n - 1 ? 0 : 1);
        ASSERT(wrong == 0);
        Mle again = Mle::new_(n_vars, t).unwrap();
        ASSERT(again.batch_inverse_in_place().unwrap() == 4);
        ASSERT(again == mi);
        ASSERT(Mle::new_(0, ints({-1})).unwrap().batch_inverse().unwrap().evaluation_slice() == ints({-1}));
        // running products
        Fr total;
        const Mle s = Mle::new_(2, ints({2, 3, 4, 5})).unwrap();
        ASSERT(s.prefix_product(false, &total).unwrap().evaluation_slice() == ints({1, 2, 6, 24}) && total == Fr::from(120));
        ASSERT(s.prefix_product(true).unwrap().evaluation_slice() == ints({2, 6, 24, 120}));
        Mle z = Mle::new_(2, ints({2, 0, 4, 5})).unwrap();
        ASSERT(z.prefix_product(true, &total).unwrap().evaluation_slice() == ints({2, 0, 0, 0}) && total == Fr::from(0));
        ASSERT(z.prefix_product_in_place(false).unwrap() == Fr::from(0));
        ASSERT(z.evaluation_slice() == ints({1, 2, 0, 0}));
        // the inverse of the running product is the running product of the inverses
        for (size_t i = 0; i < n; ++i) t[i] = Fr::from(3 * i + 2);
        mt = Mle::new_(n_vars, t).unwrap();
        ASSERT(mt.batch_inverse().unwrap().prefix_product(true).unwrap() == mt.prefix_product(true).unwrap().batch_inverse().unwrap());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: batch inverse host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
