// UnivariatePolynomial through the C++ host mirror (zk_amd/host/zk.hpp): the reference's KATs (univariate_poly.rs:257-319 with
// small integers) and one 2^20-point product against values the driving test passes in (argv[1]/{a,b,c}.bin: little-endian u64
// limbs, 4 per element).  Built and run by tests/test_gpu_upoly.py and tests/test_upoly_host.py (needs a gfx950 device to run).
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Poly = UnivariatePolynomial<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static Poly from_ints(std::initializer_list<uint64_t> v) {
    std::vector<Fr> c;
    for (uint64_t x : v) c.push_back(Fr::from(x));
    return Poly::new_(c);
}
static std::vector<Fr> read_elems(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    f.seekg(0, std::ios::end);
    const size_t n = (size_t)f.tellg() / 32;
    f.seekg(0);
    std::vector<Fr> v(n);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * 32));
    return v;
}

int main(int argc, char **argv) {
    try {
        // test_polynomial_multiplication
        const Poly p = from_ints({4, 3, 2}), q = from_ints({3, 4, 0, 4});
        ASSERT((p * q) == from_ints({12, 25, 18, 24, 12, 8}));
        ASSERT((p * q) == (q * p));
        ASSERT((from_ints({}) * from_ints({0, 2})).len() == 0);
        ASSERT((from_ints({0, 2}) * from_ints({})).len() == 0);
        ASSERT((from_ints({0}) * from_ints({1, 2, 3})) == from_ints({0, 0, 0}));
        ASSERT((p * p) == from_ints({16, 24, 25, 12, 4}));
        // test_evaluation
        ASSERT(from_ints({0, 2}).evaluate(Fr::from(4)) == Fr::from(8));
        ASSERT(from_ints({}).evaluate(Fr::from(4)) == Fr::from(0));
        ASSERT(p.coefficients() == from_ints({4, 3, 2}).coefficients());   // operands unchanged
        if (argc > 1) {
            const std::string dir = argv[1];
            const Poly a = Poly::new_(read_elems(dir + "/a.bin")), b = Poly::new_(read_elems(dir + "/b.bin"));
            const std::vector<Fr> want = read_elems(dir + "/c.bin");
            const Poly c = a * b;
            ASSERT(c.len() == a.len() + b.len() - 1);
            ASSERT(c.coefficients() == want);
            const Fr z = Fr::from(0x1234567);
            ASSERT(c.evaluate(z) == Poly::new_(want).evaluate(z));
        }
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: upoly host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
