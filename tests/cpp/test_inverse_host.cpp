// Host-side check of the batch inversion's single field inverse (zk_amd/csrc/inv_field.cuh compiled for the CPU, no GPU needed):
// fe_inverse_binary, the binary extended Euclidean inverse, must equal the host's Fermat inverse fe_inverse bit for bit and satisfy
// a * a^-1 = 1 -- 5000 random elements plus edge values (1, 2, p - 1, p - 2, R, R^2, powers of two and their neighbours) per field, all
// three fields; zero stays zero.  Built with clang++ (field.cuh uses __builtin_addc).  Driven by tests/test_batch_inverse_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../zk_amd/csrc/host_field.hpp"
#include "../../zk_amd/csrc/inv_field.cuh"
using namespace zk;
static uint64_t sm(uint64_t &x) {
    uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
int main() {
    int bad = 0;
    for (int f = 0; f < 3; ++f) {
        const FieldParams &P = field_info(f)->P;
        uint64_t st = 77 + f;
        auto below_p = [&](const Fe &c) { Fe d; return sub8(d.v, c.v, P.p) != 0; };
        auto rnd = [&]() {
            Fe c;
            do {
                for (int i = 0; i < 4; ++i) {
                    const uint64_t x = sm(st);
                    c.v[2 * i] = (uint32_t)x, c.v[2 * i + 1] = (uint32_t)(x >> 32);
                }
                if (P.bits & 31) c.v[7] &= (1u << (P.bits & 31)) - 1;
            } while (!below_p(c) || fe_is_zero(c));
            return c;
        };
        std::vector<Fe> cases;
        Fe one_int = {{1, 0, 0, 0, 0, 0, 0, 0}}, two_int = {{2, 0, 0, 0, 0, 0, 0, 0}}, pm1, pm2, r1, r2;
        sub8(pm1.v, P.p, one_int.v);
        sub8(pm2.v, P.p, two_int.v);
        for (int i = 0; i < 8; ++i) r1.v[i] = P.r1[i], r2.v[i] = P.r2[i];
        for (const Fe &e : {one_int, two_int, pm1, pm2, r1, r2}) cases.push_back(e);   // as stored integers: every limb pattern counts
        for (uint32_t k = 1; k < P.bits; ++k) {
            Fe e = fe_zero();
            e.v[k >> 5] = 1u << (k & 31);
            if (!below_p(e)) continue;
            Fe m, q;
            sub8(m.v, e.v, one_int.v);
            add8(q.v, e.v, one_int.v);
            cases.push_back(e);
            cases.push_back(m);
            if (below_p(q)) cases.push_back(q);
        }
        for (int it = 0; it < 5000; ++it) cases.push_back(rnd());
        for (size_t i = 0; i < cases.size(); ++i) {
            const Fe a = cases[i], want = fe_inverse(a, P), got = fe_inverse_binary(a, P);
            if (!fe_eq(want, got) || !fe_eq(fe_mul(a, got, P), fe_one(P))) {
                if (bad < 5) std::printf("MISMATCH field %d case %zu\n", f, i);
                ++bad;
            }
        }
        if (!fe_is_zero(fe_inverse_binary(fe_zero(), P))) ++bad, std::printf("zero did not stay zero, field %d\n", f);
        std::printf("field %d: %zu inverses ok\n", f, cases.size());
    }
    std::printf(bad ? "FAILED %d\n" : "ok: binary inverse equals the Fermat inverse%.0d\n", bad);
    return bad != 0;
}
