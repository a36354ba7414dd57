// The batch multilinear commitment through the C++ host mirror (zk_amd/host/zk.hpp: MlBatch<F>::commit / root / open / verify /
// proof_bytes / lincomb / eq_sums_many): openings whose values are the tables' evaluations and whose one proof the host verifier
// accepts, several openings of one commitment, the verifier's verdicts after a changed value, point, root, seed or byte, the length
// formula, the root of one table against MlPcs's, the linear combination and the per-point sums against evaluations, and the error
// codes.  Built and run by tests/test_gpu_mlbatch.py (needs a gfx950 device to run).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;
using Rows = std::vector<std::vector<Fr>>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    try {
        const Fr one = Fr::from(1), five = Fr::from(5), zero = Fr::from(0), minus_one = Fr::from_i64(-1);
        const uint32_t n = 10, k = 3;
        // C = A + B entry by entry, over the integers: what the linear combinations below are held against
        std::vector<Fr> a((size_t)1 << n), b(a.size()), c(a.size());
        for (size_t i = 0; i < a.size(); ++i) a[i] = Fr::from(3 * i * i + 7 * i + 1), b[i] = Fr::from(11 * i + 5), c[i] = Fr::from(3 * i * i + 18 * i + 6);
        const std::vector<Mle> tables = {Mle::new_(n, a).unwrap(), Mle::new_(n, b).unwrap(), Mle::new_(n, c).unwrap()};
        Digest seed{};
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(13 * i + 1);
        std::vector<Fr> z1(n), z2(n);
        for (uint32_t j = 0; j < n; ++j) z1[j] = Fr::from(1000003ull * j + 17), z2[j] = j % 3 == 0 ? zero : j % 3 == 1 ? one : minus_one;
        const Rows one_point = {z1}, two_points = {z1, z2}, six_points = {z1, z2, z2, z1, z2, z1};   // more points than one pass takes
        struct Shape {
            uint32_t b, f, q;
        };
        const Shape shapes[] = {{1, 0, 8}, {2, 3, 8}, {3, 1, 1}};
        for (const Shape &sh : shapes) {
            const MlBatch<F> com = std::move(MlBatch<F>::commit(tables, sh.b, five).unwrap());
            ASSERT(com.n_vars() == n && com.n_tables() == k);
            const Digest root = com.root();
            const uint32_t R = n - sh.f;
            uint64_t want = 32ull * (3 * R + R - 1 + (1ull << sh.f)) + 32ull * sh.q * (2 * k + n + sh.b - 1);
            for (uint32_t r = 1; r < R; ++r) want += 32ull * sh.q * (2 + n + sh.b - 1 - r);
            for (const Rows *zs : {&one_point, &two_points, &six_points, &one_point}) {   // several openings of one commitment
                const uint32_t m = (uint32_t)zs->size();
                ASSERT(MlBatch<F>::proof_bytes(n, k, m, sh.b, sh.f, sh.q).unwrap() == want);
                const MlBatchOpening<F> o = com.open(*zs, sh.f, sh.q, seed).unwrap();
                ASSERT(o.proof.size() == want && o.values.size() == m);
                for (uint32_t j = 0; j < m; ++j)
                    for (uint32_t t = 0; t < k; ++t) ASSERT(o.values[j][t] == tables[t].evaluate((*zs)[j]).unwrap());
                ASSERT(MlBatch<F>::verify(root, *zs, o.values, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                ASSERT(com.open(*zs, sh.f, sh.q, seed).unwrap().proof == o.proof);   // the same bytes again
                Rows other_values = o.values;
                other_values[m - 1][k - 1] = one;
                ASSERT(!MlBatch<F>::verify(root, *zs, other_values, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                other_values = o.values;
                std::swap(other_values[0][0], other_values[0][1]);   // two tables' values exchanged
                ASSERT(!MlBatch<F>::verify(root, *zs, other_values, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                Rows other_points = *zs;
                other_points[m - 1][n - 1] = Fr::from(77);
                ASSERT(!MlBatch<F>::verify(root, other_points, o.values, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                Digest other = root;
                other[5] ^= 2;
                ASSERT(!MlBatch<F>::verify(other, *zs, o.values, o.proof, sh.b, sh.f, sh.q, five, seed).unwrap());
                other = seed;
                other[0] ^= 1;
                ASSERT(!MlBatch<F>::verify(root, *zs, o.values, o.proof, sh.b, sh.f, sh.q, five, other).unwrap());
                ASSERT(!MlBatch<F>::verify(root, *zs, o.values, o.proof, sh.b, sh.f, sh.q, one, seed).unwrap());   // another shift
                for (size_t at : {(size_t)3, o.proof.size() / 2, o.proof.size() - 40, o.proof.size() - 1}) {
                    std::vector<uint8_t> bad = o.proof;
                    bad[at] ^= 0x04;
                    ASSERT(!MlBatch<F>::verify(root, *zs, o.values, bad, sh.b, sh.f, sh.q, five, seed).unwrap());
                }
                std::vector<uint8_t> cut(o.proof.begin(), o.proof.end() - 1), longer = o.proof;
                longer.push_back(0);
                ASSERT(MlBatch<F>::verify(root, *zs, o.values, cut, sh.b, sh.f, sh.q, five, seed).is_err());      // another length
                ASSERT(MlBatch<F>::verify(root, *zs, o.values, longer, sh.b, sh.f, sh.q, five, seed).is_err());
            }
            ASSERT(com.root() == root);   // the handle survives its openings
            ASSERT(com.open(one_point, n, sh.q, seed).is_err());   // log_final >= n_vars
            ASSERT(com.open(one_point, sh.f, 0, seed).is_err());
            ASSERT(com.open(Rows{std::vector<Fr>(n - 1, one)}, sh.f, sh.q, seed).is_err());   // a point of another arity
            ASSERT(com.open(Rows(17, z1), sh.f, sh.q, seed).is_err() && com.open(Rows{}, sh.f, sh.q, seed).is_err());
            // one table alone: MlPcs's root
            ASSERT(MlBatch<F>::commit({tables[1]}, sh.b, five).unwrap().root() == MlPcs<F>::commit(tables[1], sh.b, five).unwrap().root());
        }
        ASSERT(tables[0].evaluation_slice() == a && tables[2].evaluation_slice() == c);   // the tables are left intact
        // the linear combination: A + B = C, A + B - C = 0, one table picked out
        ASSERT(MlBatch<F>::lincomb({tables[0], tables[1]}, {one, one}).unwrap().evaluation_slice() == c);
        ASSERT(MlBatch<F>::lincomb(tables, {one, one, minus_one}).unwrap().evaluation_slice() == std::vector<Fr>(a.size(), zero));
        ASSERT(MlBatch<F>::lincomb(tables, {zero, one, zero}).unwrap().evaluation_slice() == b);
        ASSERT(MlBatch<F>::lincomb(tables, {one, one}).is_err() && MlBatch<F>::lincomb({}, {}).is_err());
        ASSERT(MlBatch<F>::lincomb({tables[0], Mle::new_(n - 1, std::vector<Fr>(a.size() / 2, one)).unwrap()}, {one, one}).is_err());
        // the per-point sums are MlPcs::eq_sums's at every tail, which are the evaluations at z_0 = 0 and z_0 = 1
        Rows tails;
        for (const std::vector<Fr> &z : six_points) tails.emplace_back(z.begin() + 1, z.end());
        const std::vector<std::array<Fr, 2>> sums = MlBatch<F>::eq_sums_many(tables[0], tails).unwrap();
        ASSERT(sums.size() == tails.size());
        for (size_t j = 0; j < tails.size(); ++j) {
            const std::array<Fr, 2> single = MlPcs<F>::eq_sums(tables[0], tails[j]).unwrap();
            std::vector<Fr> at0 = six_points[j];
            at0[0] = zero;
            ASSERT(sums[j] == single && sums[j][0] == tables[0].evaluate(at0).unwrap());
        }
        ASSERT(MlBatch<F>::eq_sums_many(tables[0], Rows{z1}).is_err());   // a tail has n_vars - 1 elements
        ASSERT(MlBatch<F>::eq_sums_many(tables[0], Rows(17, tails[0])).is_err());
        // parameters that do not fit
        ASSERT(MlBatch<F>::commit(tables, 0, five).is_err() && MlBatch<F>::commit(tables, 9, five).is_err() && MlBatch<F>::commit(tables, 2, zero).is_err());
        ASSERT(MlBatch<F>::commit({}, 1, five).is_err());
        ASSERT(MlBatch<F>::commit({tables[0], Mle::new_(n - 1, std::vector<Fr>(a.size() / 2, one)).unwrap()}, 1, five).is_err());   // two sizes
        ASSERT(MlBatch<F>::proof_bytes(0, 1, 1, 1, 0, 8).is_err() && MlBatch<F>::proof_bytes(4, 1, 1, 1, 4, 8).is_err());
        ASSERT(MlBatch<F>::proof_bytes(4, 0, 1, 1, 0, 8).is_err() && MlBatch<F>::proof_bytes(4, 257, 1, 1, 0, 8).is_err());
        ASSERT(MlBatch<F>::proof_bytes(4, 1, 0, 1, 0, 8).is_err() && MlBatch<F>::proof_bytes(4, 1, 17, 1, 0, 8).is_err());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: mlbatch host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
