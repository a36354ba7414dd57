// The algebra of the dense coefficient-form multilinear polynomial through the C++ host mirror (zk_amd/host/zk.hpp): the reference's
// own vectors (coefficient_form.rs tests :691-1000, :1192-1245) on polynomials with every key present -- partial_evaluate, the repeated
// and the over-long assignment, the two selector errors with their texts, relabel, scalar_multiply, Add and Mul.  Built and run by
// tests/test_gpu_cmle_algebra.py and tests/test_cmle_algebra_host.py (needs a gfx950 device to run).
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Cmle = CoeffMultilinearPolynomial<F>;
using Assignment = std::pair<std::vector<bool>, Fr>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static std::vector<Fr> ints(std::initializer_list<int64_t> v) {
    std::vector<Fr> c;
    for (int64_t x : v) c.push_back(Fr::from_i64(x));
    return c;
}
static Assignment assign(size_t n, size_t v, int64_t value) {
    std::vector<bool> s(n, false);
    s[v] = true;
    return {s, Fr::from_i64(value)};
}
// 5ab + 7bc + 8d with every key present (:691-702): keys 3, 6 and 8
static Cmle poly_5ab_7bc_8d() { return Cmle::upload(4, ints({0, 0, 0, 5, 0, 0, 7, 0, 8, 0, 0, 0, 0, 0, 0, 0})).unwrap(); }

int main() {
    try {
        Cmle p = poly_5ab_7bc_8d();
        // :712-746  a = 2, b = 3 -> 30 + 21c + 8d, then c = 2 -> 72 + 8d
        Cmle q = p.partial_evaluate({assign(4, 1, 3), assign(4, 0, 2)}).unwrap();
        ASSERT(q.n_vars() == 4 && q.fixed_mask() == 3 && q.len() == 4);
        ASSERT(q.coefficients() == ints({30, 21, 8, 0}));   // keys 0, 4 (c), 8 (d), 12 (cd)
        Cmle q2 = q.partial_evaluate({assign(4, 2, 2)}).unwrap();
        ASSERT(q2.fixed_mask() == 7 && q2.coefficients() == ints({72, 8}));
        ASSERT(p.fixed_mask() == 0 && p.coefficients().size() == 16);   // out of place
        // :748-800  all four assigned, and a assigned twice: the first one counts
        Cmle all = p.partial_evaluate({assign(4, 0, 2), assign(4, 0, 3), assign(4, 1, 4), assign(4, 2, 3), assign(4, 3, 5)}).unwrap();
        ASSERT(all.fixed_mask() == 15 && all.coefficients() == ints({164}));
        ASSERT(all.evaluate_slice(ints({9, 9, 9, 9})).unwrap() == Fr::from_i64(164));
        // :802-809  a selector longer than n_vars is ignored; :705-709 no assignment is a copy
        ASSERT(p.partial_evaluate({assign(5, 0, 3)}).unwrap().coefficients() == p.coefficients());
        ASSERT(p.partial_evaluate({}).unwrap().coefficients() == p.coefficients());
        auto e1 = p.partial_evaluate({assign(3, 0, 3)});
        ASSERT(e1.is_err() && std::string(e1.err()) == "the selector array len should be the same as the number of variables");
        auto e2 = p.partial_evaluate({{std::vector<bool>{true, false, true, false}, Fr::from(1)}});
        ASSERT(e2.is_err() && std::string(e2.err()) == "only select single variable, cannot get indexes for constant or multiple variables");
        // :1192-1245  2ab + 3cd + 5acd + 6bd at b = 1, c = 1 -> 2a + 9d + 5ad, relabelled 2a + 9b + 5ab
        Cmle r = Cmle::upload(4, ints({0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 6, 0, 3, 5, 0, 0})).unwrap();
        Cmle s = r.partial_evaluate({assign(4, 1, 1), assign(4, 2, 1)}).unwrap();
        ASSERT(s.n_vars() == 4 && s.coefficients() == ints({0, 2, 9, 5}));
        ASSERT(s.to_evaluation_form().is_err());
        Cmle t = s.relabel().unwrap();
        ASSERT(t.n_vars() == 2 && t.fixed_mask() == 0 && t.coefficients() == ints({0, 2, 9, 5}));
        ASSERT(t.to_evaluation_form().is_ok());
        // :843-881  Add and scalar_multiply, and Mul by a polynomial of no variable
        const std::vector<Fr> twice = ints({0, 0, 0, 10, 0, 0, 14, 0, 16, 0, 0, 0, 0, 0, 0, 0});
        ASSERT((p + p).unwrap().coefficients() == twice);
        ASSERT(p.scalar_multiply(Fr::from(2)).unwrap().coefficients() == twice);
        Cmle two = Cmle::upload(0, ints({2})).unwrap();
        ASSERT((p * two).unwrap().coefficients() == twice && (two * p).unwrap().n_vars() == 4);
        ASSERT((q + p).is_err() && (q * p).is_err());   // a partially evaluated operand
        // :883-922  5ab * 6c = 30abc
        Cmle ab = Cmle::upload(2, ints({0, 0, 0, 5})).unwrap(), c6 = Cmle::upload(1, ints({0, 6})).unwrap();
        Cmle abc = (ab * c6).unwrap();
        ASSERT(abc.n_vars() == 3 && abc.coefficients() == ints({0, 0, 0, 0, 0, 0, 0, 30}));
        const std::vector<uint8_t> b = q.to_bytes();
        ASSERT(b.size() == 4 + 40 * 4 && b[3] == 4 && b[4 + 40 + 7] == 4 && b[4 + 40 + 39] == 21 && b[4 + 80 + 7] == 8);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        if (std::string(e.what()).find("no usable gfx950") != std::string::npos) {
            std::printf("no CPU fallback\n");
            return 2;
        }
        return 1;
    }
    if (failures) return 1;
    std::printf("test_cmle_algebra: ok\n");
    return 0;
}
