// The dense coefficient-form multilinear polynomial through the C++ host mirror (zk_amd/host/zk.hpp): the reference's
// test_interpolation KAT (coefficient_form.rs:1105-1137), evaluate_slice, its error text, to_evaluation_form and to_bytes.  Built and
// run by tests/test_gpu_cmle.py and tests/test_cmle_host.py (needs a gfx950 device to run).
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Cmle = CoeffMultilinearPolynomial<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static std::vector<Fr> ints(std::initializer_list<int64_t> v) {
    std::vector<Fr> c;
    for (int64_t x : v) c.push_back(Fr::from_i64(x));
    return c;
}

int main() {
    try {
        auto table = MultiLinearPolynomial<F>::new_(2, ints({2, 4, 8, 3})).unwrap();
        auto poly = Cmle::interpolate(table).unwrap();
        ASSERT(poly.n_vars() == 2);
        ASSERT(poly.coefficients() == ints({2, 6, 2, -7}));
        ASSERT(poly.evaluate_slice(ints({0, 1})).unwrap() == Fr::from_i64(4));
        ASSERT(poly.evaluate_slice(ints({1, 0})).unwrap() == Fr::from_i64(8));
        ASSERT(poly.evaluate_slice(ints({1, 1, 9})).unwrap() == Fr::from_i64(3));
        auto err = poly.evaluate_slice(ints({1}));
        ASSERT(err.is_err() && std::string(err.err()) == "evaluate requires an assignment for every variable");
        ASSERT(poly.to_evaluation_form().unwrap() == table);
        const std::vector<uint8_t> b = poly.to_bytes();
        ASSERT(b.size() == 4 + 40 * 4 && b[3] == 2 && b[4 + 40 + 7] == 1 && b[4 + 40 + 39] == 6);
        ASSERT(Cmle::upload(2, ints({1, 2, 3})).is_err());
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        if (std::string(e.what()).find("no usable gfx950") != std::string::npos) {
            std::printf("no CPU fallback\n");
            return 2;
        }
        return 1;
    }
    if (failures) return 1;
    std::printf("test_cmle: ok\n");
    return 0;
}
