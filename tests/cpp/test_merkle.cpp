// Merkle commitments through the C++ host mirror (zk_amd/host/zk.hpp: MerkleTree::commit / root / level / open, zk::merkle_verify):
// the tree of two columns of 2^5 rows against the definition written out here over zk_keccak256 (leaf = hash of the rows' 32-byte
// big-endian canonical images, node = hash of the two children), the one-row tree, openings with and without rows, the host
// verifier's verdicts after one flipped bit, the move semantics and the error codes.  Built and run by tests/test_gpu_merkle.py (needs a
// gfx950 device to run).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../zk_amd/host/zk.hpp"

using namespace zk;
using F = Bn254Fr;
using Fr = Fe<F>;
using Mle = MultiLinearPolynomial<F>;

static int failures = 0;
#define ASSERT(cond) do { if (!(cond)) { std::printf("  ASSERT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static void be32(const Fr &e, uint8_t out[32]) {
    uint64_t c[4];
    zk_fe_to_canonical(F::id, e.l.data(), c);
    for (int b = 0; b < 32; ++b) out[b] = (uint8_t)(c[3 - b / 8] >> (8 * (7 - b % 8)));
}
static Digest hash(const std::vector<uint8_t> &msg) {
    Digest d{};
    zk_keccak256(msg.data(), msg.size(), d.data());
    return d;
}
static Digest leaf_of(const std::vector<Fr> &row) {
    std::vector<uint8_t> msg(32 * row.size());
    for (size_t j = 0; j < row.size(); ++j) be32(row[j], msg.data() + 32 * j);
    return hash(msg);
}
static Digest node_of(const Digest &l, const Digest &r) {
    std::vector<uint8_t> msg(64);
    std::memcpy(msg.data(), l.data(), 32);
    std::memcpy(msg.data() + 32, r.data(), 32);
    return hash(msg);
}

int main() {
    try {
        const uint32_t n = 5, k = 2;
        const size_t rows = (size_t)1 << n;
        std::vector<Fr> a(rows), b(rows);
        for (size_t i = 0; i < rows; ++i) {
            a[i] = Fr::from_i64((int64_t)i - 3);        // -3 .. : p - 3, p - 2, p - 1, 0, 1, ...
            b[i] = Fr::from(i * i + 7);
        }
        const std::vector<Mle> cols = {Mle::new_(n, a).unwrap(), Mle::new_(n, b).unwrap()};
        MerkleTree<F> tree = std::move(MerkleTree<F>::commit(cols).unwrap());
        ASSERT(tree.n_vars() == n && tree.n_columns() == k);
        // the definition
        std::vector<std::vector<Digest>> levels(n + 1);
        for (size_t i = 0; i < rows; ++i) levels[0].push_back(leaf_of({a[i], b[i]}));
        for (uint32_t d = 1; d <= n; ++d)
            for (size_t j = 0; j < rows >> d; ++j) levels[d].push_back(node_of(levels[d - 1][2 * j], levels[d - 1][2 * j + 1]));
        ASSERT(tree.root() == levels[n][0]);
        for (uint32_t d = 0; d <= n; ++d) ASSERT(tree.level(d).unwrap() == levels[d]);
        ASSERT(tree.level(n + 1).is_err());
        ASSERT(cols[0].evaluation_slice() == a && cols[1].evaluation_slice() == b);   // the columns are unchanged
        // openings: first, last, a duplicate, out of order
        const std::vector<uint64_t> idx = {0, rows - 1, 9, 9, 16};
        MerkleOpening<F> o = tree.open(idx, cols).unwrap();
        MerkleOpening<F> quiet = tree.open(idx).unwrap();
        ASSERT(o.rows.size() == idx.size() * k && o.paths.size() == idx.size() * n && quiet.rows.empty() && quiet.paths == o.paths);
        for (size_t q = 0; q < idx.size(); ++q) {
            const uint64_t i = idx[q];
            ASSERT(o.rows[q * k] == a[i] && o.rows[q * k + 1] == b[i]);
            for (uint32_t d = 0; d < n; ++d) ASSERT(o.paths[q * n + d] == levels[d][(i >> d) ^ 1]);
            const std::vector<Fr> row = {o.rows[q * k], o.rows[q * k + 1]};
            const Digest *path = &o.paths[q * n];
            ASSERT(merkle_verify<F>(tree.root(), n, i, row, path).unwrap());
            ASSERT(!merkle_verify<F>(tree.root(), n, i ^ 4, row, path).unwrap());         // another index
            ASSERT(!merkle_verify<F>(tree.root(), n, i, {row[1], row[0]}, path).unwrap()); // the row in the wrong order
            std::vector<Digest> bent(path, path + n);
            bent[q % n][q] ^= 0x10;
            ASSERT(!merkle_verify<F>(tree.root(), n, i, row, bent.data()).unwrap());       // one flipped bit in the path
            Digest root = tree.root();
            root[31] ^= 1;
            ASSERT(!merkle_verify<F>(root, n, i, row, path).unwrap());                     // ... in the root
        }
        ASSERT(tree.open({}).unwrap().paths.empty());
        ASSERT(tree.open({rows}).is_err());                                                // an index out of range
        ASSERT(tree.open({0}, {cols[0]}).is_err());                                        // another number of columns
        ASSERT(merkle_verify<F>(tree.root(), n, rows, {a[0], b[0]}, o.paths.data()).is_err());
        // one row: the root is the leaf, the path is empty
        const Mle single = Mle::new_(0, {Fr::from(0)}).unwrap();
        MerkleTree<F> tiny = std::move(MerkleTree<F>::commit({single}).unwrap());
        ASSERT(tiny.n_vars() == 0 && tiny.root() == leaf_of({Fr::from(0)}));
        ASSERT(merkle_verify<F>(tiny.root(), 0, 0, {Fr::from(0)}, nullptr).unwrap());
        ASSERT(!merkle_verify<F>(tiny.root(), 0, 0, {Fr::from(1)}, nullptr).unwrap());
        // moves hand the tree on; a second commitment of the same columns has the same root
        const Digest before = tree.root();
        MerkleTree<F> moved = std::move(tree);
        ASSERT(tree.raw() == nullptr && moved.root() == before);
        tiny = std::move(moved);
        ASSERT(tiny.root() == before && tiny.n_vars() == n);
        ASSERT(MerkleTree<F>::commit(cols).unwrap().root() == before);
        // mixed sizes and no columns are refused
        ASSERT(MerkleTree<F>::commit({cols[0], single}).is_err());
        ASSERT(MerkleTree<F>::commit({}).is_err());
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok: merkle host tests passed%.0d\n", failures);
    return failures ? 1 : 0;
}
