// Sharding by index mod world through the C++ host mirror (zk_amd/host/zk.hpp): MultiLinearPolynomial::new_shard, split and
// interleave against the host's own strided reading of the table.  Built and run by tests/test_shard_layout_host.py (it
// compiles this file into a temporary directory; needs a gfx950 device to run).
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    try {
        const size_t n = 10, N = (size_t)1 << n;
        std::vector<Fr> evals;
        for (size_t i = 0; i < N; ++i) evals.push_back(Fr::from(7 * i + 3));
        Mle t = Mle::new_(n, evals).unwrap();
        for (uint32_t world : {1u, 2u, 8u, 16u, 64u, 128u, 1024u}) {
            std::vector<Mle> shards = t.split(world).unwrap();
            ASSERT(shards.size() == world);
            for (uint32_t g = 0; g < world; ++g) {
                ASSERT(shards[g].n_vars() == n - __builtin_ctz(world));
                const std::vector<Fr> got = shards[g].evaluation_slice();
                bool same = got.size() == N / world;
                for (size_t j = 0; same && j < got.size(); ++j) same = got[j] == evals[j * world + g];
                ASSERT(same);
                ASSERT(Mle::new_shard(n, evals, world, g).unwrap() == shards[g]);
            }
            ASSERT(Mle::interleave(shards).unwrap() == t);
        }
        ASSERT(t.evaluation_slice() == evals);   // split leaves its input alone
        ASSERT(t.split(3).is_err());
        ASSERT(t.split(2048).is_err());
        ASSERT(Mle::new_shard(n, evals, 8, 8).is_err());
        ASSERT(std::string(Mle::new_shard(n + 1, evals, 2, 0).err()) == "evaluation vec len should equal 2^n_vars");
        std::vector<Mle> uneven = t.split(2).unwrap();
        uneven.push_back(t.split(4).unwrap()[0]);
        uneven.push_back(t.split(4).unwrap()[1]);
        ASSERT(Mle::interleave(uneven).is_err());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: shard layout host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
