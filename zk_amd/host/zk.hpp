// zk.hpp -- C++17 host-side mirror of the reference's public API for the hot path, over the C ABI (include/zk_amd.h).
//
// The reference is Rust; the image has no Rust toolchain, so this header is the compiled-language host side: the same
// type and method names, argument meaning and error behaviour as
//   polynomial::multilinear::evaluation_form::MultiLinearPolynomial<F>   evaluation_form.rs:7-103
//   polynomial::product_poly::ProductPoly<F>                             product_poly.rs:7-88
//   sumcheck::prover::SumcheckProver<MAX_VAR_DEGREE, F>                  prover.rs:9-73
//   sumcheck::verifier::SumcheckVerifier<F>                              verifier.rs:9-78
//   transcript::Transcript                                               transcript/src/lib.rs:5-35
//   fft::{fft, ifft}                                                     fft/src/lib.rs:4-19
//   polynomial::univariate_poly::UnivariatePolynomial<F> (new, coefficients, evaluate, Mul)   univariate_poly.rs:7-40,186-209
// `Result<T, &'static str>` is zk::Result<T> (value or the reference's message); `F` is a field tag type.  Tables stay
// resident on the GPU behind the handle; `evaluation_slice()` downloads.  bindings/rust/ is the same thing in Rust.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/zk_amd.h"

namespace zk {

struct Bn254Fr { static constexpr int32_t id = ZK_FIELD_BN254_FR; };
struct Bls12_381Fr { static constexpr int32_t id = ZK_FIELD_BLS12_381_FR; };
struct Bls12_377Fr { static constexpr int32_t id = ZK_FIELD_BLS12_377_FR; };

// a field element exactly as ark-ff stores it: 4 LE u64 limbs, Montgomery form
template <class F>
struct Fe {
    std::array<uint64_t, 4> l{};
    static Fe from(uint64_t v) {   // F::from(v)
        Fe e;
        zk_fe_from_u64(F::id, v, e.l.data());
        return e;
    }
    static Fe from_i64(int64_t v) {   // Fr::from(-2) in the reference's tests
        if (v >= 0) return from((uint64_t)v);
        uint64_t p[4], c[4];
        zk_field_modulus(F::id, p);
        uint64_t borrow = (uint64_t)(-v);   // p - |v|
        for (int i = 0; i < 4; ++i) {
            c[i] = p[i] - borrow;
            borrow = p[i] < borrow ? 1 : 0;
        }
        Fe e;
        zk_fe_from_canonical(F::id, c, e.l.data());
        return e;
    }
    bool operator==(const Fe &o) const { return l == o.l; }
    bool operator!=(const Fe &o) const { return !(*this == o); }
};

// Result<T, &'static str>
template <class T>
class Result {
    std::unique_ptr<T> v_;
    const char *err_ = nullptr;

public:
    Result(T v) : v_(new T(std::move(v))) {}
    Result(int32_t status) : err_(zk_strerror(status)) {}
    bool is_ok() const { return err_ == nullptr; }
    bool is_err() const { return err_ != nullptr; }
    const char *err() const { return err_; }
    T &unwrap() {
        if (err_) throw std::runtime_error(std::string("called `Result::unwrap()` on an `Err` value: ") + err_);
        return *v_;
    }
    T &expect(const char *msg) {
        if (err_) throw std::runtime_error(std::string(msg) + ": " + err_);
        return *v_;
    }
};

// one device context per field tag (the reference has no such notion: arithmetic is ambient)
template <class F>
inline zk_ctx *context() {
    static zk_ctx *ctx = [] {
        zk_ctx *c = nullptr;
        const int32_t rc = zk_ctx_create(F::id, 0, &c);
        if (rc != ZK_OK) throw std::runtime_error(std::string("zk_ctx_create: ") + zk_strerror(rc));
        return c;
    }();
    return ctx;
}

template <class F>
class MultiLinearPolynomial {
    struct Handle {
        zk_mle *h = nullptr;
        ~Handle() { if (h) zk_mle_free(context<F>(), h); }
    };
    std::shared_ptr<Handle> h_;
    explicit MultiLinearPolynomial(zk_mle *h) : h_(std::make_shared<Handle>()) { h_->h = h; }
    template <class> friend class ProductPoly;
    template <uint8_t, class> friend class SumcheckProver;
    template <class> friend class Circuit;
    template <class> friend class CoeffMultilinearPolynomial;
    template <class> friend struct Fri;
    template <class> friend struct GrandProduct;
    template <class> friend struct FractionalSum;
    template <class> friend struct Permutation;

public:
    // evaluation_form.rs:15-27
    static Result<MultiLinearPolynomial> new_(size_t n_vars, const std::vector<Fe<F>> &evaluations) {
        zk_mle *h = nullptr;
        const int32_t rc = zk_mle_upload(context<F>(), n_vars, reinterpret_cast<const uint64_t *>(evaluations.data()),
                                         evaluations.size(), &h);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial(h);
    }
    // sharding by index mod world (include/zk_amd.h, zk_mle_upload_shard / _split / _interleave): rank g holds
    // {idx : idx mod world == g} with local index idx / world -- the layout of the sharded prover and NTT
    static Result<MultiLinearPolynomial> new_shard(size_t n_vars, const std::vector<Fe<F>> &evaluations, uint32_t world, uint32_t rank) {
        zk_mle *h = nullptr;
        const int32_t rc = zk_mle_upload_shard(context<F>(), n_vars, reinterpret_cast<const uint64_t *>(evaluations.data()),
                                               evaluations.size(), world, rank, &h);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial(h);
    }
    Result<std::vector<MultiLinearPolynomial>> split(uint32_t world) const {
        std::vector<zk_mle *> hs(world ? world : 1, nullptr);
        const int32_t rc = zk_mle_split(context<F>(), h_->h, world, hs.data());
        if (rc != ZK_OK) return rc;
        std::vector<MultiLinearPolynomial> out;
        for (uint32_t g = 0; g < world; ++g) out.push_back(MultiLinearPolynomial(hs[g]));
        return out;
    }
    static Result<MultiLinearPolynomial> interleave(const std::vector<MultiLinearPolynomial> &shards) {
        std::vector<const zk_mle *> hs;
        for (auto &s : shards) hs.push_back(s.raw());
        zk_mle *h = nullptr;
        const int32_t rc = zk_mle_interleave(context<F>(), hs.data(), (uint32_t)hs.size(), &h);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial(h);
    }
    size_t n_vars() const {   // :30
        uint64_t n = 0;
        zk_mle_n_vars(h_->h, &n);
        return (size_t)n;
    }
    // :40-80
    Result<MultiLinearPolynomial> partial_evaluate(size_t initial_var, const std::vector<Fe<F>> &assignments) const {
        zk_mle *o = nullptr;
        const int32_t rc = zk_mle_partial_evaluate(context<F>(), h_->h, initial_var,
                                                   reinterpret_cast<const uint64_t *>(assignments.data()), assignments.size(), &o);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial(o);
    }
    // :83-89
    Result<Fe<F>> evaluate(const std::vector<Fe<F>> &assignments) const {
        Fe<F> out;
        const int32_t rc = zk_mle_evaluate(context<F>(), h_->h, reinterpret_cast<const uint64_t *>(assignments.data()),
                                           assignments.size(), out.l.data());
        if (rc != ZK_OK) return rc;
        return out;
    }
    // :92-94 (downloads)
    std::vector<Fe<F>> evaluation_slice() const {
        std::vector<Fe<F>> v((size_t)1 << n_vars());
        zk_mle_download(context<F>(), h_->h, reinterpret_cast<uint64_t *>(v.data()));
        return v;
    }
    // :97-103
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> b((size_t)32 << n_vars());
        zk_mle_to_bytes(context<F>(), h_->h, b.data());
        return b;
    }
    // batch inversion and running products (the reference has none; include/zk_amd.h, zk_mle_batch_inverse / zk_mle_prefix_product)
    static Result<MultiLinearPolynomial> alloc(size_t n_vars) {
        zk_mle *h = nullptr;
        const int32_t rc = zk_mle_alloc(context<F>(), n_vars, &h);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial(h);
    }
    // a new table of 1 / (t[i] + shift), zero where the denominator is zero; *zeros (optional) = how many there were (waits)
    Result<MultiLinearPolynomial> batch_inverse(const Fe<F> *shift = nullptr, uint64_t *zeros = nullptr) const {
        Result<MultiLinearPolynomial> out = alloc(n_vars());
        if (out.is_err()) return out;
        const int32_t rc = zk_mle_batch_inverse(context<F>(), h_->h, shift ? shift->l.data() : nullptr, out.unwrap().h_->h, zeros);
        if (rc != ZK_OK) return rc;
        return out;
    }
    // the same in place
    Result<uint64_t> batch_inverse_in_place(const Fe<F> *shift = nullptr) {
        uint64_t zeros = 0;
        const int32_t rc = zk_mle_batch_inverse(context<F>(), h_->h, shift ? shift->l.data() : nullptr, h_->h, &zeros);
        if (rc != ZK_OK) return rc;
        return zeros;
    }
    // exclusive: out[0] = 1, out[i] = t[0] ... t[i-1]; inclusive: out[i] = t[0] ... t[i]; *total (optional) = the product of all (waits)
    Result<MultiLinearPolynomial> prefix_product(bool inclusive = false, Fe<F> *total = nullptr) const {
        Result<MultiLinearPolynomial> out = alloc(n_vars());
        if (out.is_err()) return out;
        const int32_t rc = zk_mle_prefix_product(context<F>(), h_->h, inclusive ? 1 : 0, out.unwrap().h_->h, total ? total->l.data() : nullptr);
        if (rc != ZK_OK) return rc;
        return out;
    }
    Result<Fe<F>> prefix_product_in_place(bool inclusive = false) {
        Fe<F> total;
        const int32_t rc = zk_mle_prefix_product(context<F>(), h_->h, inclusive ? 1 : 0, h_->h, total.l.data());
        if (rc != ZK_OK) return rc;
        return total;
    }
    bool operator==(const MultiLinearPolynomial &o) const {   // #[derive(PartialEq)]: compared on the device (zk_mle_equal)
        int32_t eq = 0;
        if (zk_mle_equal(context<F>(), h_->h, o.h_->h, &eq) != ZK_OK) return false;
        return eq != 0;
    }
    zk_mle *raw() const { return h_->h; }
};

// polynomial::univariate_poly::UnivariatePolynomial (univariate_poly.rs:7-12): coefficients lowest degree first, resident on the
// GPU.  The reference's new / evaluate / Mul cannot fail; a library error (no device, or a product past the supported transform
// length: include/zk_amd.h, zk_upoly_mul) is thrown as std::runtime_error.
template <class F>
class UnivariatePolynomial {
    struct Handle {
        zk_upoly *h = nullptr;
        ~Handle() { if (h) zk_upoly_free(context<F>(), h); }
    };
    std::shared_ptr<Handle> h_;
    explicit UnivariatePolynomial(zk_upoly *h) : h_(std::make_shared<Handle>()) { h_->h = h; }
    static void ok(int32_t rc, const char *what) {
        if (rc != ZK_OK) throw std::runtime_error(std::string(what) + ": " + zk_strerror(rc));
    }

public:
    // :16-19
    static UnivariatePolynomial new_(const std::vector<Fe<F>> &coefficients) {
        zk_upoly *h = nullptr;
        ok(zk_upoly_upload(context<F>(), reinterpret_cast<const uint64_t *>(coefficients.data()), coefficients.size(), &h), "zk_upoly_upload");
        return UnivariatePolynomial(h);
    }
    size_t len() const {
        uint64_t n = 0;
        zk_upoly_len(h_->h, &n);
        return (size_t)n;
    }
    // :21-23 (downloads)
    std::vector<Fe<F>> coefficients() const {
        std::vector<Fe<F>> v(len());
        ok(zk_upoly_download(context<F>(), h_->h, reinterpret_cast<uint64_t *>(v.data())), "zk_upoly_download");
        return v;
    }
    // :29-40
    Fe<F> evaluate(const Fe<F> &x) const {
        Fe<F> out;
        ok(zk_upoly_evaluate(context<F>(), h_->h, x.l.data(), out.l.data()), "zk_upoly_evaluate");
        return out;
    }
    // Mul for &UnivariatePolynomial :186-209
    UnivariatePolynomial operator*(const UnivariatePolynomial &o) const {
        zk_upoly *h = nullptr;
        ok(zk_upoly_mul(context<F>(), h_->h, o.h_->h, &h), "zk_upoly_mul");
        return UnivariatePolynomial(h);
    }
    // Add for &UnivariatePolynomial :157-184
    UnivariatePolynomial operator+(const UnivariatePolynomial &o) const {
        zk_upoly *h = nullptr;
        ok(zk_upoly_add(context<F>(), h_->h, o.h_->h, &h), "zk_upoly_add");
        return UnivariatePolynomial(h);
    }
    // ::interpolate :43-49 (xs = 0 .. n-1)
    static UnivariatePolynomial interpolate(const std::vector<Fe<F>> &ys) {
        const UnivariatePolynomial y = new_(ys);
        zk_upoly *h = nullptr;
        ok(zk_upoly_interpolate(context<F>(), y.h_->h, &h), "zk_upoly_interpolate");
        return UnivariatePolynomial(h);
    }
    // ::interpolate_xy :54-80; where the reference panics (a repeated x, :68) this throws with the library's message
    static UnivariatePolynomial interpolate_xy(const std::vector<Fe<F>> &xs, const std::vector<Fe<F>> &ys) {
        const UnivariatePolynomial x = new_(xs), y = new_(ys);
        zk_upoly *h = nullptr;
        ok(zk_upoly_interpolate_xy(context<F>(), x.h_->h, y.h_->h, &h), "zk_upoly_interpolate_xy");
        return UnivariatePolynomial(h);
    }
    // ::evaluate :29-40 at every point of xs (a polynomial used as a vector of points): a device vector of xs.len() values, no host wait
    UnivariatePolynomial evaluate_many(const UnivariatePolynomial &xs) const {
        zk_upoly *h = nullptr;
        ok(zk_upoly_evaluate_many(context<F>(), h_->h, xs.h_->h, &h), "zk_upoly_evaluate_many");
        return UnivariatePolynomial(h);
    }
    std::vector<Fe<F>> evaluate_many(const std::vector<Fe<F>> &xs) const { return evaluate_many(new_(xs)).coefficients(); }
    // division with remainder (the reference has none; include/zk_amd.h, zk_upoly_divrem): {q, r} with *this = q b + r, len(q) =
    // len - len(b) + 1 and len(r) = len(b) - 1, nothing trimmed; b's last coefficient is inverted (zero: the PANIC_INVERSE error)
    std::pair<UnivariatePolynomial, UnivariatePolynomial> divrem(const UnivariatePolynomial &b) const {
        zk_upoly *q = nullptr, *r = nullptr;
        ok(zk_upoly_divrem(context<F>(), h_->h, b.h_->h, &q, &r), "zk_upoly_divrem");
        return {UnivariatePolynomial(q), UnivariatePolynomial(r)};
    }
    UnivariatePolynomial operator/(const UnivariatePolynomial &b) const {
        zk_upoly *q = nullptr;
        ok(zk_upoly_divrem(context<F>(), h_->h, b.h_->h, &q, nullptr), "zk_upoly_divrem");
        return UnivariatePolynomial(q);
    }
    UnivariatePolynomial operator%(const UnivariatePolynomial &b) const {
        zk_upoly *r = nullptr;
        ok(zk_upoly_divrem(context<F>(), h_->h, b.h_->h, nullptr, &r), "zk_upoly_divrem");
        return UnivariatePolynomial(r);
    }
    // the k coefficients of 1 / *this mod z^k
    UnivariatePolynomial inverse_series(uint64_t k) const {
        zk_upoly *h = nullptr;
        ok(zk_upoly_inverse_series(context<F>(), h_->h, k, &h), "zk_upoly_inverse_series");
        return UnivariatePolynomial(h);
    }
    // a new vector of 1 / (v[i] + shift), zero where the denominator is zero (zk_upoly_batch_inverse); *zeros (optional) = how many (waits)
    UnivariatePolynomial batch_inverse(const Fe<F> *shift = nullptr, uint64_t *zeros = nullptr) const {
        zk_upoly *h = nullptr;
        ok(zk_upoly_batch_inverse(context<F>(), h_->h, shift ? shift->l.data() : nullptr, &h, zeros), "zk_upoly_batch_inverse");
        return UnivariatePolynomial(h);
    }
    bool operator==(const UnivariatePolynomial &o) const { return coefficients() == o.coefficients(); }   // #[derive(PartialEq)]
    zk_upoly *raw() const { return h_->h; }
};

// value-semantics batch inversion (zk_batch_inverse_host): 1 / (values[i] + shift), zeros left zero; *zeros (optional) = how many
template <class F>
inline std::vector<Fe<F>> batch_inverse(const std::vector<Fe<F>> &values, const Fe<F> *shift = nullptr, uint64_t *zeros = nullptr) {
    std::vector<Fe<F>> out(values.size());
    const int32_t rc = zk_batch_inverse_host(context<F>(), reinterpret_cast<const uint64_t *>(values.data()), values.size(),
                                             shift ? shift->l.data() : nullptr, reinterpret_cast<uint64_t *>(out.data()), zeros);
    if (rc != ZK_OK) throw std::runtime_error(std::string("zk_batch_inverse_host: ") + zk_strerror(rc));
    return out;
}

// Binary Keccak-256 Merkle commitment over k tables of 2^n elements with every level on the GPU (zk_merkle; the reference has none,
// include/zk_amd.h has the format).  Move-only: the object owns the device tree.
using Digest = std::array<uint8_t, 32>;
template <class F>
struct MerkleOpening {
    std::vector<Fe<F>> rows;     // n_queries x n_columns, query-major (empty when no columns were given)
    std::vector<Digest> paths;   // n_queries x n_vars, the siblings bottom up
};
template <class F>
class MerkleTree {
    zk_merkle *h_ = nullptr;
    explicit MerkleTree(zk_merkle *h) : h_(h) {}
    static std::vector<const zk_mle *> raws(const std::vector<MultiLinearPolynomial<F>> &columns) {
        std::vector<const zk_mle *> hs;
        for (auto &col : columns) hs.push_back(col.raw());
        return hs;
    }

public:
    MerkleTree(MerkleTree &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    MerkleTree &operator=(MerkleTree &&o) noexcept {
        if (this != &o) {
            zk_merkle_free(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    MerkleTree(const MerkleTree &) = delete;
    MerkleTree &operator=(const MerkleTree &) = delete;
    ~MerkleTree() { zk_merkle_free(h_); }
    // stream-ordered, no host wait; the tree does not refer to the columns afterwards
    static Result<MerkleTree> commit(const std::vector<MultiLinearPolynomial<F>> &columns) {
        const std::vector<const zk_mle *> hs = raws(columns);
        zk_merkle *h = nullptr;
        const int32_t rc = zk_merkle_commit(context<F>(), hs.data(), (uint32_t)hs.size(), &h);
        if (rc != ZK_OK) return rc;
        return MerkleTree(h);
    }
    uint32_t n_vars() const {
        uint32_t n = 0;
        zk_merkle_n_vars(h_, &n);
        return n;
    }
    uint32_t n_columns() const {
        uint32_t k = 0;
        zk_merkle_n_columns(h_, &k);
        return k;
    }
    Digest root() const {
        Digest d{};
        const int32_t rc = zk_merkle_root(context<F>(), h_, d.data());
        if (rc != ZK_OK) throw std::runtime_error(std::string("zk_merkle_root: ") + zk_strerror(rc));
        return d;
    }
    Result<std::vector<Digest>> level(uint32_t d) const {
        if (d > n_vars()) return (int32_t)ZK_ERR_BAD_ARG;
        std::vector<Digest> out((size_t)1 << (n_vars() - d));
        const int32_t rc = zk_merkle_level(context<F>(), h_, d, out[0].data());
        if (rc != ZK_OK) return rc;
        return out;
    }
    // the openings of the rows `indices`; columns empty: the paths only
    Result<MerkleOpening<F>> open(const std::vector<uint64_t> &indices, const std::vector<MultiLinearPolynomial<F>> &columns = {}) const {
        const std::vector<const zk_mle *> hs = raws(columns);
        MerkleOpening<F> o;
        o.paths.resize(indices.size() * n_vars());
        if (!hs.empty()) o.rows.resize(indices.size() * n_columns());
        const int32_t rc = zk_merkle_open(context<F>(), h_, hs.empty() ? nullptr : hs.data(), (uint32_t)hs.size(), indices.data(), indices.size(),
                                          reinterpret_cast<uint64_t *>(o.rows.data()), reinterpret_cast<uint8_t *>(o.paths.data()));
        if (rc != ZK_OK) return rc;
        return o;
    }
    zk_merkle *raw() const { return h_; }
};
// host only (zk_merkle_verify_host): does `path` (n_vars digests, bottom up) lead from the leaf of `row` at `index` to `root`?
template <class F>
inline Result<bool> merkle_verify(const Digest &root, uint32_t n_vars, uint64_t index, const std::vector<Fe<F>> &row, const Digest *path) {
    int32_t ok = 0;
    const int32_t rc = zk_merkle_verify_host(F::id, root.data(), n_vars, (uint32_t)row.size(), index, reinterpret_cast<const uint64_t *>(row.data()),
                                             reinterpret_cast<const uint8_t *>(path), &ok);
    if (rc != ZK_OK) return rc;
    return ok != 0;
}

// FRI low-degree proofs (zk_fri_*; the reference has none, include/zk_amd.h has the protocol and the proof format): log_degree d,
// log_blowup b, log_arity a, log_final f, n_queries Q, a non-zero shift and a 32-byte seed
struct FriParams {
    uint32_t log_degree, log_blowup, log_arity, log_final, n_queries;
};
template <class F>
struct Fri {
    // the evaluations of p over shift * <root_of_unity(2^log_n)>, natural order
    static Result<MultiLinearPolynomial<F>> lde(const UnivariatePolynomial<F> &p, uint32_t log_n, const Fe<F> &shift) {
        zk_mle *h = nullptr;
        const int32_t rc = zk_fri_lde(context<F>(), p.raw(), log_n, shift.l.data(), &h);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial<F>(h);
    }
    // `layer` over the coset of `shift`, folded by 2^log_arity at beta: a new table of n_vars - log_arity variables
    static Result<MultiLinearPolynomial<F>> fold(const MultiLinearPolynomial<F> &layer, uint32_t log_arity, const Fe<F> &shift, const Fe<F> &beta) {
        if (layer.n_vars() < log_arity) return (int32_t)ZK_ERR_EVAL_LEN;
        Result<MultiLinearPolynomial<F>> out = MultiLinearPolynomial<F>::alloc(layer.n_vars() - log_arity);
        if (out.is_err()) return out;
        const int32_t rc = zk_fri_fold(context<F>(), layer.raw(), log_arity, shift.l.data(), beta.l.data(), out.unwrap().raw());
        if (rc != ZK_OK) return rc;
        return out;
    }
    static Result<uint64_t> proof_bytes(const FriParams &fp) {
        uint64_t n = 0;
        const int32_t rc = zk_fri_proof_bytes(fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries, &n);
        if (rc != ZK_OK) return rc;
        return n;
    }
    static Result<std::vector<uint8_t>> prove(const UnivariatePolynomial<F> &p, const FriParams &fp, const Fe<F> &shift, const Digest &seed) {
        Result<uint64_t> n = proof_bytes(fp);
        if (n.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        std::vector<uint8_t> proof(n.unwrap());
        const int32_t rc = zk_fri_prove(context<F>(), p.raw(), fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries, shift.l.data(),
                                        seed.data(), proof.data());
        if (rc != ZK_OK) return rc;
        return proof;
    }
    // host only (zk_fri_verify_host)
    static Result<bool> verify(const std::vector<uint8_t> &proof, const FriParams &fp, const Fe<F> &shift, const Digest &seed) {
        int32_t ok = 0;
        const int32_t rc = zk_fri_verify_host(F::id, fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries, shift.l.data(), seed.data(),
                                              proof.data(), proof.size(), &ok);
        if (rc != ZK_OK) return rc;
        return ok != 0;
    }
};

// FRI polynomial commitment (zk_pcs_*, zk_deep_quotient; the reference has none, include/zk_amd.h has the protocol and the proof format):
// one commitment to k polynomials of at most 2^log_degree coefficients, opened at any number of points, one after another
template <class F>
struct PcsOpening {
    std::vector<Fe<F>> values;    // f_c(z): the public claim
    std::vector<uint8_t> proof;
};
template <class F>
class Pcs {
    zk_pcs *h_ = nullptr;
    FriParams fp_{};   // log_degree, log_blowup, log_arity of the commitment; log_final and n_queries belong to an opening
    Fe<F> shift_{};
    Pcs(zk_pcs *h, const FriParams &fp, const Fe<F> &shift) : h_(h), fp_(fp), shift_(shift) {}

public:
    Pcs(Pcs &&o) noexcept : h_(o.h_), fp_(o.fp_), shift_(o.shift_) { o.h_ = nullptr; }
    Pcs &operator=(Pcs &&o) noexcept {
        if (this != &o) {
            zk_pcs_free(h_);
            h_ = o.h_, fp_ = o.fp_, shift_ = o.shift_;
            o.h_ = nullptr;
        }
        return *this;
    }
    Pcs(const Pcs &) = delete;
    Pcs &operator=(const Pcs &) = delete;
    ~Pcs() { zk_pcs_free(h_); }
    // stream-ordered, no host wait; the handle does not refer to the polynomials afterwards
    static Result<Pcs> commit(const std::vector<UnivariatePolynomial<F>> &polys, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity,
                              const Fe<F> &shift) {
        std::vector<const zk_upoly *> hs;
        for (auto &p : polys) hs.push_back(p.raw());
        zk_pcs *h = nullptr;
        const int32_t rc = zk_pcs_commit(context<F>(), hs.data(), (uint32_t)hs.size(), log_degree, log_blowup, log_arity, shift.l.data(), &h);
        if (rc != ZK_OK) return rc;
        return Pcs(h, FriParams{log_degree, log_blowup, log_arity, 0, 0}, shift);
    }
    uint32_t n_polys() const {
        uint32_t k = 0;
        zk_pcs_n_polys(h_, &k);
        return k;
    }
    Digest root() const {
        Digest d{};
        const int32_t rc = zk_pcs_root(context<F>(), h_, d.data());
        if (rc != ZK_OK) throw std::runtime_error(std::string("zk_pcs_root: ") + zk_strerror(rc));
        return d;
    }
    static Result<uint64_t> proof_bytes(uint32_t k, const FriParams &fp) {
        uint64_t n = 0;
        const int32_t rc = zk_pcs_proof_bytes(k, fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries, &n);
        if (rc != ZK_OK) return rc;
        return n;
    }
    // the values at z and the proof that they are right; the commitment is left intact
    Result<PcsOpening<F>> open(const Fe<F> &z, uint32_t log_final, uint32_t n_queries, const Digest &seed) const {
        const uint32_t k = n_polys();
        Result<uint64_t> n = proof_bytes(k, FriParams{fp_.log_degree, fp_.log_blowup, fp_.log_arity, log_final, n_queries});
        if (n.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        PcsOpening<F> o;
        o.values.resize(k);
        o.proof.resize(n.unwrap());
        const int32_t rc = zk_pcs_open(context<F>(), h_, z.l.data(), log_final, n_queries, seed.data(), reinterpret_cast<uint64_t *>(o.values.data()),
                                       o.proof.data());
        if (rc != ZK_OK) return rc;
        return o;
    }
    // host only (zk_pcs_verify_host)
    static Result<bool> verify(const Digest &root, const Fe<F> &z, const std::vector<Fe<F>> &values, const std::vector<uint8_t> &proof, const FriParams &fp,
                               const Fe<F> &shift, const Digest &seed) {
        int32_t ok = 0;
        const int32_t rc = zk_pcs_verify_host(F::id, (uint32_t)values.size(), fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries,
                                              shift.l.data(), seed.data(), root.data(), z.l.data(), reinterpret_cast<const uint64_t *>(values.data()),
                                              proof.data(), proof.size(), &ok);
        if (rc != ZK_OK) return rc;
        return ok != 0;
    }
    // out[i] = (sum_c alpha^c (columns[c][i] - values[c])) / (shift w^i - z) over the columns' coset, as a new table (zk_deep_quotient)
    static Result<MultiLinearPolynomial<F>> deep_quotient(const std::vector<MultiLinearPolynomial<F>> &columns, const Fe<F> &shift, const Fe<F> &z,
                                                          const std::vector<Fe<F>> &values, const Fe<F> &alpha) {
        if (columns.empty() || values.size() != columns.size()) return (int32_t)ZK_ERR_BAD_ARG;
        std::vector<const zk_mle *> hs;
        for (auto &col : columns) hs.push_back(col.raw());
        Result<MultiLinearPolynomial<F>> out = MultiLinearPolynomial<F>::alloc(columns[0].n_vars());
        if (out.is_err()) return out;
        const int32_t rc = zk_deep_quotient(context<F>(), hs.data(), (uint32_t)hs.size(), shift.l.data(), z.l.data(),
                                            reinterpret_cast<const uint64_t *>(values.data()), alpha.l.data(), out.unwrap().raw());
        if (rc != ZK_OK) return rc;
        return out;
    }
    zk_pcs *raw() const { return h_; }
};

// Multilinear polynomial commitment (zk_mlpcs_*, zk_mle_eq_sums; the reference has none, include/zk_amd.h has the protocol and the proof
// format): one commitment to a table, opened at any number of points, one after another
template <class F>
struct MlPcsOpening {
    Fe<F> value;    // t(point): the public claim
    std::vector<uint8_t> proof;
};
template <class F>
class MlPcs {
    zk_mlpcs *h_ = nullptr;
    uint32_t log_blowup_ = 0;
    MlPcs(zk_mlpcs *h, uint32_t log_blowup) : h_(h), log_blowup_(log_blowup) {}

public:
    MlPcs(MlPcs &&o) noexcept : h_(o.h_), log_blowup_(o.log_blowup_) { o.h_ = nullptr; }
    MlPcs &operator=(MlPcs &&o) noexcept {
        if (this != &o) {
            zk_mlpcs_free(h_);
            h_ = o.h_, log_blowup_ = o.log_blowup_;
            o.h_ = nullptr;
        }
        return *this;
    }
    MlPcs(const MlPcs &) = delete;
    MlPcs &operator=(const MlPcs &) = delete;
    ~MlPcs() { zk_mlpcs_free(h_); }
    // stream-ordered, no host wait; the handle does not refer to the table afterwards
    static Result<MlPcs> commit(const MultiLinearPolynomial<F> &table, uint32_t log_blowup, const Fe<F> &shift) {
        zk_mlpcs *h = nullptr;
        const int32_t rc = zk_mlpcs_commit(context<F>(), table.raw(), log_blowup, shift.l.data(), &h);
        if (rc != ZK_OK) return rc;
        return MlPcs(h, log_blowup);
    }
    uint32_t n_vars() const {
        uint32_t n = 0;
        zk_mlpcs_n_vars(h_, &n);
        return n;
    }
    Digest root() const {
        Digest d{};
        const int32_t rc = zk_mlpcs_root(context<F>(), h_, d.data());
        if (rc != ZK_OK) throw std::runtime_error(std::string("zk_mlpcs_root: ") + zk_strerror(rc));
        return d;
    }
    static Result<uint64_t> proof_bytes(uint32_t n_vars, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries) {
        uint64_t n = 0;
        const int32_t rc = zk_mlpcs_proof_bytes(n_vars, log_blowup, log_final, n_queries, &n);
        if (rc != ZK_OK) return rc;
        return n;
    }
    // the value at the point and the proof that it is right; the commitment is left intact
    Result<MlPcsOpening<F>> open(const std::vector<Fe<F>> &point, uint32_t log_final, uint32_t n_queries, const Digest &seed) const {
        if (point.size() != n_vars()) return (int32_t)ZK_ERR_EVAL_ARITY;
        Result<uint64_t> n = proof_bytes(n_vars(), log_blowup_, log_final, n_queries);
        if (n.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        MlPcsOpening<F> o;
        o.proof.resize(n.unwrap());
        const int32_t rc = zk_mlpcs_open(context<F>(), h_, reinterpret_cast<const uint64_t *>(point.data()), point.size(), log_final, n_queries,
                                         seed.data(), o.value.l.data(), o.proof.data());
        if (rc != ZK_OK) return rc;
        return o;
    }
    // host only (zk_mlpcs_verify_host)
    static Result<bool> verify(const Digest &root, const std::vector<Fe<F>> &point, const Fe<F> &value, const std::vector<uint8_t> &proof,
                               uint32_t log_blowup, uint32_t log_final, uint32_t n_queries, const Fe<F> &shift, const Digest &seed) {
        int32_t ok = 0;
        const int32_t rc = zk_mlpcs_verify_host(F::id, (uint32_t)point.size(), log_blowup, log_final, n_queries, shift.l.data(), seed.data(), root.data(),
                                                reinterpret_cast<const uint64_t *>(point.data()), value.l.data(), proof.data(), proof.size(), &ok);
        if (rc != ZK_OK) return rc;
        return ok != 0;
    }
    // S_X = sum_x' table[X 2^(n-1) + x'] eq(x', tail), X = 0, 1 (zk_mle_eq_sums); tail: n_vars - 1 elements
    static Result<std::array<Fe<F>, 2>> eq_sums(const MultiLinearPolynomial<F> &table, const std::vector<Fe<F>> &tail) {
        if (tail.size() + 1 != table.n_vars()) return (int32_t)ZK_ERR_BAD_ARG;
        std::array<Fe<F>, 2> out{};
        const int32_t rc = zk_mle_eq_sums(context<F>(), table.raw(), tail.empty() ? nullptr : reinterpret_cast<const uint64_t *>(tail.data()),
                                          reinterpret_cast<uint64_t *>(out.data()));
        if (rc != ZK_OK) return rc;
        return out;
    }
    zk_mlpcs *raw() const { return h_; }
};

// Batch multilinear commitment (zk_mlbatch_*, zk_mle_lincomb, zk_mle_eq_sums_many; the reference has none, include/zk_amd.h has the protocol
// and the proof format): k tables of one size under one tree, every opening shows all of them at m points with one proof.  Tables of
// another size go into another commitment.
template <class F>
struct MlBatchOpening {
    std::vector<std::vector<Fe<F>>> values;   // values[j][c] = t_c(points[j]): the public claims
    std::vector<uint8_t> proof;
};
template <class F>
class MlBatch {
    zk_mlbatch *h_ = nullptr;
    uint32_t log_blowup_ = 0;
    MlBatch(zk_mlbatch *h, uint32_t log_blowup) : h_(h), log_blowup_(log_blowup) {}
    static std::vector<uint64_t> flat(const std::vector<std::vector<Fe<F>>> &rows) {
        std::vector<uint64_t> out;
        for (const auto &row : rows)
            for (const Fe<F> &e : row) out.insert(out.end(), e.l.begin(), e.l.end());
        return out;
    }
    static std::vector<const zk_mle *> raws(const std::vector<MultiLinearPolynomial<F>> &tables) {
        std::vector<const zk_mle *> out;
        for (const auto &t : tables) out.push_back(t.raw());
        return out;
    }

public:
    MlBatch(MlBatch &&o) noexcept : h_(o.h_), log_blowup_(o.log_blowup_) { o.h_ = nullptr; }
    MlBatch &operator=(MlBatch &&o) noexcept {
        if (this != &o) {
            zk_mlbatch_free(h_);
            h_ = o.h_, log_blowup_ = o.log_blowup_;
            o.h_ = nullptr;
        }
        return *this;
    }
    MlBatch(const MlBatch &) = delete;
    MlBatch &operator=(const MlBatch &) = delete;
    ~MlBatch() { zk_mlbatch_free(h_); }
    // stream-ordered, no host wait; the handle does not refer to the tables afterwards
    static Result<MlBatch> commit(const std::vector<MultiLinearPolynomial<F>> &tables, uint32_t log_blowup, const Fe<F> &shift) {
        if (tables.empty()) return (int32_t)ZK_ERR_BAD_ARG;
        const std::vector<const zk_mle *> raw = raws(tables);
        zk_mlbatch *h = nullptr;
        const int32_t rc = zk_mlbatch_commit(context<F>(), raw.data(), (uint32_t)raw.size(), log_blowup, shift.l.data(), &h);
        if (rc != ZK_OK) return rc;
        return MlBatch(h, log_blowup);
    }
    uint32_t n_vars() const {
        uint32_t n = 0;
        zk_mlbatch_n_vars(h_, &n);
        return n;
    }
    uint32_t n_tables() const {
        uint32_t k = 0;
        zk_mlbatch_n_tables(h_, &k);
        return k;
    }
    Digest root() const {
        Digest d{};
        const int32_t rc = zk_mlbatch_root(context<F>(), h_, d.data());
        if (rc != ZK_OK) throw std::runtime_error(std::string("zk_mlbatch_root: ") + zk_strerror(rc));
        return d;
    }
    static Result<uint64_t> proof_bytes(uint32_t n_vars, uint32_t n_tables, uint32_t n_points, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries) {
        uint64_t n = 0;
        const int32_t rc = zk_mlbatch_proof_bytes(n_vars, n_tables, n_points, log_blowup, log_final, n_queries, &n);
        if (rc != ZK_OK) return rc;
        return n;
    }
    // every table's value at every point and the one proof that they are right; the commitment is left intact
    Result<MlBatchOpening<F>> open(const std::vector<std::vector<Fe<F>>> &points, uint32_t log_final, uint32_t n_queries, const Digest &seed) const {
        for (const auto &z : points)
            if (z.size() != n_vars()) return (int32_t)ZK_ERR_EVAL_ARITY;
        Result<uint64_t> n = proof_bytes(n_vars(), n_tables(), (uint32_t)points.size(), log_blowup_, log_final, n_queries);
        if (n.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        const std::vector<uint64_t> pts = flat(points);
        std::vector<uint64_t> vals(4 * points.size() * n_tables());
        MlBatchOpening<F> o;
        o.proof.resize(n.unwrap());
        const int32_t rc = zk_mlbatch_open(context<F>(), h_, pts.data(), (uint32_t)points.size(), log_final, n_queries, seed.data(), vals.data(), o.proof.data());
        if (rc != ZK_OK) return rc;
        o.values.assign(points.size(), std::vector<Fe<F>>(n_tables()));
        for (size_t j = 0; j < points.size(); ++j)
            for (size_t t = 0; t < n_tables(); ++t) std::memcpy(o.values[j][t].l.data(), vals.data() + 4 * (j * n_tables() + t), 32);
        return o;
    }
    // host only (zk_mlbatch_verify_host)
    static Result<bool> verify(const Digest &root, const std::vector<std::vector<Fe<F>>> &points, const std::vector<std::vector<Fe<F>>> &values,
                               const std::vector<uint8_t> &proof, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries, const Fe<F> &shift,
                               const Digest &seed) {
        if (points.empty() || values.size() != points.size() || values[0].empty()) return (int32_t)ZK_ERR_BAD_ARG;
        for (const auto &z : points)
            if (z.size() != points[0].size()) return (int32_t)ZK_ERR_BAD_ARG;
        for (const auto &row : values)
            if (row.size() != values[0].size()) return (int32_t)ZK_ERR_BAD_ARG;
        const std::vector<uint64_t> pts = flat(points), vals = flat(values);
        int32_t ok = 0;
        const int32_t rc = zk_mlbatch_verify_host(F::id, (uint32_t)points[0].size(), (uint32_t)values[0].size(), (uint32_t)points.size(), log_blowup, log_final,
                                                  n_queries, shift.l.data(), seed.data(), root.data(), pts.data(), vals.data(), proof.data(), proof.size(), &ok);
        if (rc != ZK_OK) return rc;
        return ok != 0;
    }
    // sum_c coeffs[c] tables[c] as a new table (zk_mle_lincomb)
    static Result<MultiLinearPolynomial<F>> lincomb(const std::vector<MultiLinearPolynomial<F>> &tables, const std::vector<Fe<F>> &coeffs) {
        if (tables.empty() || coeffs.size() != tables.size()) return (int32_t)ZK_ERR_BAD_ARG;
        Result<MultiLinearPolynomial<F>> out = MultiLinearPolynomial<F>::alloc(tables[0].n_vars());
        if (out.is_err()) return (int32_t)ZK_ERR_ALLOC;
        const std::vector<const zk_mle *> raw = raws(tables);
        const int32_t rc = zk_mle_lincomb(context<F>(), raw.data(), (uint32_t)raw.size(), reinterpret_cast<const uint64_t *>(coeffs.data()), out.unwrap().raw());
        if (rc != ZK_OK) return rc;
        return std::move(out.unwrap());
    }
    // (S_0^j, S_1^j) of MlPcs::eq_sums at every tail in passes of several points (zk_mle_eq_sums_many); tails: n_vars - 1 elements each
    static Result<std::vector<std::array<Fe<F>, 2>>> eq_sums_many(const MultiLinearPolynomial<F> &table, const std::vector<std::vector<Fe<F>>> &tails) {
        for (const auto &tail : tails)
            if (tail.size() + 1 != table.n_vars()) return (int32_t)ZK_ERR_BAD_ARG;
        const std::vector<uint64_t> flat_tails = flat(tails);
        std::vector<std::array<Fe<F>, 2>> out(tails.size());
        const int32_t rc = zk_mle_eq_sums_many(context<F>(), table.raw(), flat_tails.empty() ? nullptr : flat_tails.data(), (uint32_t)tails.size(),
                                               reinterpret_cast<uint64_t *>(out.data()));
        if (rc != ZK_OK) return rc;
        return out;
    }
    zk_mlbatch *raw() const { return h_; }
};

// Grand-product argument (zk_mle_product_tree, zk_gprod_*; the reference has none, include/zk_amd.h has the protocol and the proof format):
// P = prod_i (t[i] + shift) shown to a verifier who is left with the one claim t(point) = claim.  The seed must bind the table.
template <class F>
struct GrandProductProof {
    Fe<F> product;                 // P: the public claim
    std::vector<uint8_t> proof;
    std::vector<Fe<F>> point;      // what the verifier derives: t(point) = claim is left to check
    Fe<F> claim;
};
template <class F>
struct GrandProductClaim {
    bool ok = false;               // false: the proof is rejected, point and claim are empty
    std::vector<Fe<F>> point;
    Fe<F> claim;
};
template <class F>
struct GrandProduct {
    static Result<uint64_t> proof_bytes(uint32_t n_vars) {
        uint64_t n = 0;
        const int32_t rc = zk_gprod_proof_bytes(n_vars, &n);
        if (rc != ZK_OK) return rc;
        return n;
    }
    // the product tree in heap order: out[0] = 1, out[2^j + i] = V_j[i], out[1] = P; stream-ordered, no host wait
    static Result<MultiLinearPolynomial<F>> tree(const MultiLinearPolynomial<F> &table, const Fe<F> *shift = nullptr) {
        zk_mle *h = nullptr;
        const int32_t rc = zk_mle_product_tree(context<F>(), table.raw(), shift ? shift->l.data() : nullptr, &h);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial<F>(h);
    }
    // one host wait for the whole proof; the table is left intact
    static Result<GrandProductProof<F>> prove(const MultiLinearPolynomial<F> &table, const Digest &seed, const Fe<F> *shift = nullptr) {
        Result<uint64_t> n = proof_bytes((uint32_t)table.n_vars());
        if (n.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        GrandProductProof<F> o;
        o.proof.resize(n.unwrap());
        o.point.resize(table.n_vars());
        const int32_t rc = zk_gprod_prove(context<F>(), table.raw(), shift ? shift->l.data() : nullptr, seed.data(), o.product.l.data(), o.proof.data(),
                                          reinterpret_cast<uint64_t *>(o.point.data()), o.claim.l.data());
        if (rc != ZK_OK) return rc;
        return o;
    }
    // host only (zk_gprod_verify_host)
    static Result<GrandProductClaim<F>> verify(uint32_t n_vars, const Digest &seed, const Fe<F> &product, const std::vector<uint8_t> &proof,
                                               const Fe<F> *shift = nullptr) {
        GrandProductClaim<F> o;
        std::vector<Fe<F>> point(n_vars ? n_vars : 1);
        int32_t ok = 0;
        const int32_t rc = zk_gprod_verify_host(F::id, n_vars, shift ? shift->l.data() : nullptr, seed.data(), product.l.data(), proof.data(), proof.size(),
                                                reinterpret_cast<uint64_t *>(point.data()), o.claim.l.data(), &ok);
        if (rc != ZK_OK) return rc;
        o.ok = ok != 0;
        if (o.ok) o.point.assign(point.begin(), point.begin() + n_vars);
        return o;
    }
    // verify plus the evaluation it leaves open, for a verifier that holds the table
    static Result<bool> verify_table(const MultiLinearPolynomial<F> &table, const Digest &seed, const Fe<F> &product, const std::vector<uint8_t> &proof,
                                     const Fe<F> *shift = nullptr) {
        Result<GrandProductClaim<F>> r = verify((uint32_t)table.n_vars(), seed, product, proof, shift);
        if (r.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        const GrandProductClaim<F> &cl = r.unwrap();
        return cl.ok && table.evaluate(cl.point).unwrap() == cl.claim;
    }
};

// Zerocheck argument (zk_gate_*, zk_zerocheck_*, zk_mle_gate_sums; the reference has none, include/zk_amd.h has the protocol and the proof
// format): G(t_0[i], .., t_{k-1}[i]) = 0 on every row for the gate G = sum_i coeff_i prod_{f in term i} x_f, shown to a verifier who is
// left with the k claims t_c(point) = claims[c], which one MultilinearBatchCommitment opening discharges.  The seed must bind the tables.
template <class F>
struct GateTerm {
    Fe<F> coeff;
    std::vector<uint32_t> columns;   // a repeat is a power, none a constant
};
template <class F>
struct Gate {   // a host object: needs no context
    Gate() = default;
    Gate(Gate &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Gate &operator=(Gate &&o) noexcept {
        if (this != &o) {
            if (h_) zk_gate_free(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    Gate(const Gate &) = delete;
    Gate &operator=(const Gate &) = delete;
    ~Gate() {
        if (h_) zk_gate_free(h_);
    }
    static Result<Gate> create(uint32_t k, const std::vector<GateTerm<F>> &terms) {
        std::vector<uint64_t> coeffs;
        std::vector<uint32_t> lens, flat;
        for (const GateTerm<F> &t : terms) {
            coeffs.insert(coeffs.end(), t.coeff.l.begin(), t.coeff.l.end());
            lens.push_back((uint32_t)t.columns.size());
            flat.insert(flat.end(), t.columns.begin(), t.columns.end());
        }
        if (terms.empty()) return (int32_t)ZK_ERR_BAD_ARG;
        if (flat.empty()) flat.push_back(0);
        zk_gate *h = nullptr;
        const int32_t rc = zk_gate_create(F::id, k, (uint32_t)terms.size(), coeffs.data(), lens.data(), flat.data(), &h);
        if (rc != ZK_OK) return rc;
        Gate g;
        g.h_ = h;
        return Result<Gate>(std::move(g));
    }
    uint32_t degree() const {
        uint32_t d = 0;
        zk_gate_degree(h_, &d);
        return d;
    }
    uint32_t n_columns() const {
        uint32_t k = 0;
        zk_gate_n_columns(h_, &k);
        return k;
    }
    zk_gate *raw() const { return h_; }

  private:
    zk_gate *h_ = nullptr;
};
template <class F>
struct ZerocheckProof {
    std::vector<uint8_t> proof;
    std::vector<Fe<F>> point;      // what the verifier derives: t_c(point) = claims[c] is left to check
    std::vector<Fe<F>> claims;
};
template <class F>
struct ZerocheckClaim {
    bool ok = false;               // false: the proof is rejected, point and claims are empty
    std::vector<Fe<F>> point, claims;
};
template <class F>
struct Zerocheck {
    static Result<uint64_t> proof_bytes(const Gate<F> &gate, uint32_t n_vars) {
        uint64_t n = 0;
        const int32_t rc = zk_zerocheck_proof_bytes(gate.raw(), n_vars, &n);
        if (rc != ZK_OK) return rc;
        return n;
    }
    static std::vector<const zk_mle *> handles(const std::vector<const MultiLinearPolynomial<F> *> &tables) {
        std::vector<const zk_mle *> hs;
        for (const MultiLinearPolynomial<F> *t : tables) hs.push_back(t ? t->raw() : nullptr);
        return hs;
    }
    // one host wait for the whole proof; the tables are left intact; the prover does not check the statement
    static Result<ZerocheckProof<F>> prove(const std::vector<const MultiLinearPolynomial<F> *> &tables, const Gate<F> &gate, const Digest &seed) {
        if (tables.size() != gate.n_columns() || !tables[0]) return (int32_t)ZK_ERR_BAD_ARG;
        Result<uint64_t> n = proof_bytes(gate, (uint32_t)tables[0]->n_vars());
        if (n.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        ZerocheckProof<F> o;
        o.proof.resize(n.unwrap());
        o.point.resize(tables[0]->n_vars());
        o.claims.resize(gate.n_columns());
        const std::vector<const zk_mle *> hs = handles(tables);
        const int32_t rc = zk_zerocheck_prove(context<F>(), hs.data(), gate.raw(), seed.data(), o.proof.data(), reinterpret_cast<uint64_t *>(o.point.data()),
                                              reinterpret_cast<uint64_t *>(o.claims.data()));
        if (rc != ZK_OK) return rc;
        return o;
    }
    // host only (zk_zerocheck_verify_host)
    static Result<ZerocheckClaim<F>> verify(const Gate<F> &gate, uint32_t n_vars, const Digest &seed, const std::vector<uint8_t> &proof) {
        ZerocheckClaim<F> o;
        std::vector<Fe<F>> point(n_vars ? n_vars : 1), claims(gate.n_columns());
        int32_t ok = 0;
        const int32_t rc = zk_zerocheck_verify_host(gate.raw(), n_vars, seed.data(), proof.data(), proof.size(), reinterpret_cast<uint64_t *>(point.data()),
                                                    reinterpret_cast<uint64_t *>(claims.data()), &ok);
        if (rc != ZK_OK) return rc;
        o.ok = ok != 0;
        if (o.ok) {
            o.point.assign(point.begin(), point.begin() + n_vars);
            o.claims = claims;
        }
        return o;
    }
    // sum_x' eq(x', tail) G(tables(X, x')) at X = 0 .. d, the tables as they are (zk_mle_gate_sums); tail: n_vars - 1 elements
    static Result<std::vector<Fe<F>>> gate_sums(const std::vector<const MultiLinearPolynomial<F> *> &tables, const Gate<F> &gate, const std::vector<Fe<F>> &tail) {
        if (tables.size() != gate.n_columns() || !tables[0] || tail.size() + 1 != tables[0]->n_vars()) return (int32_t)ZK_ERR_BAD_ARG;
        std::vector<Fe<F>> out(gate.degree() + 1);
        const std::vector<const zk_mle *> hs = handles(tables);
        const int32_t rc = zk_mle_gate_sums(context<F>(), hs.data(), gate.raw(), tail.empty() ? nullptr : reinterpret_cast<const uint64_t *>(tail.data()),
                                            reinterpret_cast<uint64_t *>(out.data()));
        if (rc != ZK_OK) return rc;
        return out;
    }
};

// Wiring (copy-constraint) permutation argument (zk_mle_perm_fingerprint, zk_perm_*; the reference has none, include/zk_amd.h has the
// protocol and the proof format): the witness columns w satisfy the wiring sigma, shown to a verifier who is left with the 2 k claims
// w_c(point) = claims[c], sigma_c(point) = claims[k + c].  The seed must bind the commitments of w and sigma; beta, gamma come after it.
template <class F>
struct PermutationProof {
    std::vector<uint8_t> proof;
    std::vector<Fe<F>> point;      // what the verifier derives: the 2 k evaluations at it are left to check
    std::vector<Fe<F>> claims;     // the w values, then the sigma values
};
template <class F>
struct PermutationClaim {
    bool ok = false;               // false: the proof is rejected, point and claims are empty
    std::vector<Fe<F>> point, claims;
};
template <class F>
struct Permutation {
    using Columns = std::vector<const MultiLinearPolynomial<F> *>;
    static Result<uint64_t> proof_bytes(uint32_t n_vars, uint32_t k) {
        uint64_t n = 0;
        const int32_t rc = zk_perm_proof_bytes(n_vars, k, &n);
        if (rc != ZK_OK) return rc;
        return n;
    }
    static std::vector<const zk_mle *> handles(const Columns &tables) {
        std::vector<const zk_mle *> hs;
        for (const MultiLinearPolynomial<F> *t : tables) hs.push_back(t ? t->raw() : nullptr);
        return hs;
    }
    // the fingerprint table of n + kappa + 1 variables (zk_mle_perm_fingerprint); stream-ordered, no host wait
    static Result<MultiLinearPolynomial<F>> fingerprint(const Columns &w, const Columns &sigma, const Fe<F> &beta, const Fe<F> &gamma) {
        if (w.empty() || w.size() != sigma.size()) return (int32_t)ZK_ERR_BAD_ARG;
        const std::vector<const zk_mle *> ws = handles(w), ss = handles(sigma);
        zk_mle *h = nullptr;
        const int32_t rc = zk_mle_perm_fingerprint(context<F>(), ws.data(), ss.data(), (uint32_t)w.size(), reinterpret_cast<const uint64_t *>(&beta),
                                                   reinterpret_cast<const uint64_t *>(&gamma), &h);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial<F>(h);
    }
    // two host waits (the grand product, then the 2 k values); the columns are left intact; the prover does not check the statement
    static Result<PermutationProof<F>> prove(const Columns &w, const Columns &sigma, const Fe<F> &beta, const Fe<F> &gamma, const Digest &seed) {
        if (w.empty() || w.size() != sigma.size() || !w[0]) return (int32_t)ZK_ERR_BAD_ARG;
        Result<uint64_t> n = proof_bytes((uint32_t)w[0]->n_vars(), (uint32_t)w.size());
        if (n.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        PermutationProof<F> o;
        o.proof.resize(n.unwrap());
        o.point.resize(w[0]->n_vars());
        o.claims.resize(2 * w.size());
        const std::vector<const zk_mle *> ws = handles(w), ss = handles(sigma);
        const int32_t rc = zk_perm_prove(context<F>(), ws.data(), ss.data(), (uint32_t)w.size(), reinterpret_cast<const uint64_t *>(&beta),
                                         reinterpret_cast<const uint64_t *>(&gamma), seed.data(), o.proof.data(),
                                         reinterpret_cast<uint64_t *>(o.point.data()), reinterpret_cast<uint64_t *>(o.claims.data()));
        if (rc != ZK_OK) return rc;
        return o;
    }
    // host only (zk_perm_verify_host)
    static Result<PermutationClaim<F>> verify(uint32_t n_vars, uint32_t k, const Fe<F> &beta, const Fe<F> &gamma, const Digest &seed,
                                              const std::vector<uint8_t> &proof) {
        if (k < 1 || k > 16) return (int32_t)ZK_ERR_BAD_ARG;
        PermutationClaim<F> o;
        std::vector<Fe<F>> point(n_vars ? n_vars : 1), claims(2 * k);
        int32_t ok = 0;
        const int32_t rc = zk_perm_verify_host(F::id, n_vars, k, reinterpret_cast<const uint64_t *>(&beta), reinterpret_cast<const uint64_t *>(&gamma),
                                               seed.data(), proof.data(), proof.size(), reinterpret_cast<uint64_t *>(point.data()),
                                               reinterpret_cast<uint64_t *>(claims.data()), &ok);
        if (rc != ZK_OK) return rc;
        o.ok = ok != 0;
        if (o.ok) {
            o.point.assign(point.begin(), point.begin() + n_vars);
            o.claims = claims;
        }
        return o;
    }
};

// Fractional-sum (LogUp) argument and lookup multiplicities (zk_mle_fraction_tree, zk_fsum_*, zk_lookup_multiplicities; the reference has
// none, include/zk_amd.h has the protocol and the proof format): N / D = sum_i p[i] / (q[i] + shift) shown to a verifier who is left with
// the two claims p(point) = p_claim, q(point) = q_claim.  p = nullptr: all ones.  The seed must bind the tables.
template <class F>
struct FractionalSumProof {
    Fe<F> numerator, denominator;  // N, D: the public claim
    std::vector<uint8_t> proof;
    std::vector<Fe<F>> point;      // what the verifier derives: p(point) = p_claim and q(point) = q_claim are left to check
    Fe<F> p_claim, q_claim;
};
template <class F>
struct FractionalSumClaim {
    bool ok = false;               // false: the proof is rejected (D = 0 included), point and claims are empty
    std::vector<Fe<F>> point;
    Fe<F> p_claim, q_claim;
};
template <class F>
struct FractionTree {
    MultiLinearPolynomial<F> p, q;   // heap order: out[2^j + i] = level j; p[1] = N, q[1] = D
};
template <class F>
struct LookupMultiplicities {
    MultiLinearPolynomial<F> m;      // m[j] = #{i : witness[i] = table[j]} for the lowest j of each value, else 0
    uint64_t missing, first_missing, duplicates;   // first_missing = 2^64 - 1: none
};
template <class F>
struct FractionalSum {
    static Result<uint64_t> proof_bytes(uint32_t n_vars) {
        uint64_t n = 0;
        const int32_t rc = zk_fsum_proof_bytes(n_vars, &n);
        if (rc != ZK_OK) return rc;
        return n;
    }
    // both heaps of the fraction tree; stream-ordered, no host wait
    static Result<FractionTree<F>> tree(const MultiLinearPolynomial<F> *p, const MultiLinearPolynomial<F> &q, const Fe<F> *shift = nullptr) {
        zk_mle *hp = nullptr, *hq = nullptr;
        const int32_t rc = zk_mle_fraction_tree(context<F>(), p ? p->raw() : nullptr, q.raw(), shift ? shift->l.data() : nullptr, &hp, &hq);
        if (rc != ZK_OK) return rc;
        return FractionTree<F>{MultiLinearPolynomial<F>(hp), MultiLinearPolynomial<F>(hq)};
    }
    // one host wait for the whole proof; the tables are left intact
    static Result<FractionalSumProof<F>> prove(const MultiLinearPolynomial<F> *p, const MultiLinearPolynomial<F> &q, const Digest &seed,
                                               const Fe<F> *shift = nullptr) {
        Result<uint64_t> n = proof_bytes((uint32_t)q.n_vars());
        if (n.is_err()) return (int32_t)ZK_ERR_BAD_ARG;
        FractionalSumProof<F> o;
        o.proof.resize(n.unwrap());
        o.point.resize(q.n_vars());
        uint64_t sum[8], claims[8];
        const int32_t rc = zk_fsum_prove(context<F>(), p ? p->raw() : nullptr, q.raw(), shift ? shift->l.data() : nullptr, seed.data(), sum, o.proof.data(),
                                         reinterpret_cast<uint64_t *>(o.point.data()), claims);
        if (rc != ZK_OK) return rc;
        std::memcpy(o.numerator.l.data(), sum, 32);
        std::memcpy(o.denominator.l.data(), sum + 4, 32);
        std::memcpy(o.p_claim.l.data(), claims, 32);
        std::memcpy(o.q_claim.l.data(), claims + 4, 32);
        return o;
    }
    // host only (zk_fsum_verify_host)
    static Result<FractionalSumClaim<F>> verify(uint32_t n_vars, bool has_p, const Digest &seed, const Fe<F> &numerator, const Fe<F> &denominator,
                                                const std::vector<uint8_t> &proof, const Fe<F> *shift = nullptr) {
        FractionalSumClaim<F> o;
        std::vector<Fe<F>> point(n_vars ? n_vars : 1);
        uint64_t sum[8], claims[8];
        std::memcpy(sum, numerator.l.data(), 32);
        std::memcpy(sum + 4, denominator.l.data(), 32);
        int32_t ok = 0;
        const int32_t rc = zk_fsum_verify_host(F::id, n_vars, has_p ? 1 : 0, shift ? shift->l.data() : nullptr, seed.data(), sum, proof.data(), proof.size(),
                                               reinterpret_cast<uint64_t *>(point.data()), claims, &ok);
        if (rc != ZK_OK) return rc;
        o.ok = ok != 0;
        if (o.ok) {
            o.point.assign(point.begin(), point.begin() + n_vars);
            std::memcpy(o.p_claim.l.data(), claims, 32);
            std::memcpy(o.q_claim.l.data(), claims + 4, 32);
        }
        return o;
    }
    // one host wait, for the three counters
    static Result<LookupMultiplicities<F>> multiplicities(const MultiLinearPolynomial<F> &table, const MultiLinearPolynomial<F> &witness) {
        zk_mle *h = nullptr;
        uint64_t missing = 0, first = 0, dup = 0;
        const int32_t rc = zk_lookup_multiplicities(context<F>(), table.raw(), witness.raw(), &h, &missing, &first, &dup);
        if (rc != ZK_OK) return rc;
        return LookupMultiplicities<F>{MultiLinearPolynomial<F>(h), missing, first, dup};
    }
};
template <class F>
inline Result<LookupMultiplicities<F>> lookup_multiplicities(const MultiLinearPolynomial<F> &table, const MultiLinearPolynomial<F> &witness) {
    return FractionalSum<F>::multiplicities(table, witness);
}

// polynomial::multilinear::coefficient_form::CoeffMultilinearPolynomial resident on the GPU (zk_cmle): the coefficients of the present
// keys in key order (key bit v <-> variable v).  upload / interpolate (coefficient_form.rs:200-216) make every key present;
// partial_evaluate removes the keys with a bit of a fixed variable, so the present keys are {k : k & fixed_mask() == 0} and
// coefficients() has len() = 2^(n_vars - popcount(fixed_mask())) entries, entry j being key pdep(j, ~fixed_mask()).  operator* keeps
// the keys the reference's Mul drops for zero coefficients (:393-395), with coefficient zero (include/zk_amd.h, DIVERGENCE).
template <class F>
class CoeffMultilinearPolynomial {
    struct Handle {
        zk_cmle *h = nullptr;
        ~Handle() { if (h) zk_cmle_free(context<F>(), h); }
    };
    std::shared_ptr<Handle> h_;
    explicit CoeffMultilinearPolynomial(zk_cmle *h) : h_(std::make_shared<Handle>()) { h_->h = h; }

public:
    // the dense vector itself: len != 2^n_vars -> Err
    static Result<CoeffMultilinearPolynomial> upload(size_t n_vars, const std::vector<Fe<F>> &dense) {
        zk_cmle *h = nullptr;
        const int32_t rc = zk_cmle_upload(context<F>(), n_vars, reinterpret_cast<const uint64_t *>(dense.data()), dense.size(), &h);
        if (rc != ZK_OK) return rc;
        return CoeffMultilinearPolynomial(h);
    }
    // ::interpolate :200-216 of a resident table (one value: n_vars 1)
    static Result<CoeffMultilinearPolynomial> interpolate(const MultiLinearPolynomial<F> &values) {
        zk_cmle *h = nullptr;
        const int32_t rc = zk_cmle_interpolate(context<F>(), values.raw(), &h);
        if (rc != ZK_OK) return rc;
        return CoeffMultilinearPolynomial(h);
    }
    size_t n_vars() const {
        uint64_t n = 0;
        zk_cmle_n_vars(h_->h, &n);
        return (size_t)n;
    }
    uint64_t fixed_mask() const {   // bit v set <-> variable v was fixed by partial_evaluate
        uint64_t m = 0;
        zk_cmle_fixed_mask(h_->h, &m);
        return m;
    }
    size_t len() const {   // number of present keys
        uint64_t n = 0;
        zk_cmle_len(h_->h, &n);
        return (size_t)n;
    }
    std::vector<Fe<F>> coefficients() const {   // downloads; ascending key order, index = key while fixed_mask() == 0
        std::vector<Fe<F>> v(len());
        if (zk_cmle_download(context<F>(), h_->h, reinterpret_cast<uint64_t *>(v.data())) != ZK_OK) v.clear();
        return v;
    }
    // :39-69 (fewer assignments than variables -> the reference's Err text)
    Result<Fe<F>> evaluate_slice(const std::vector<Fe<F>> &assignments) const {
        Fe<F> out;
        const int32_t rc = zk_cmle_evaluate(context<F>(), h_->h, reinterpret_cast<const uint64_t *>(assignments.data()), assignments.size(),
                                            out.l.data());
        if (rc != ZK_OK) return rc;
        return out;
    }
    // :340-347, left resident
    Result<MultiLinearPolynomial<F>> to_evaluation_form() const {
        zk_mle *o = nullptr;
        const int32_t rc = zk_cmle_to_evaluation(context<F>(), h_->h, &o);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial<F>(o);
    }
    // :131-139
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> b(4 + (size_t)40 * len());
        if (zk_cmle_to_bytes(context<F>(), h_->h, b.data()) != ZK_OK) b.clear();
        return b;
    }
    // :72-104 -- (selector, value) pairs; the reference's two selector errors come back as its own texts
    Result<CoeffMultilinearPolynomial> partial_evaluate(const std::vector<std::pair<std::vector<bool>, Fe<F>>> &assignments) const {
        std::vector<uint8_t> sel;
        std::vector<uint64_t> lens;
        std::vector<Fe<F>> vals;
        for (const auto &a : assignments) {
            lens.push_back(a.first.size());
            for (bool b : a.first) sel.push_back(b ? 1 : 0);
            vals.push_back(a.second);
        }
        zk_cmle *o = nullptr;
        const int32_t rc = zk_cmle_partial_evaluate(context<F>(), h_->h, sel.data(), lens.data(), reinterpret_cast<const uint64_t *>(vals.data()),
                                                    assignments.size(), &o);
        if (rc != ZK_OK) return rc;
        return CoeffMultilinearPolynomial(o);
    }
    // :109-123 -- the reference consumes self: relabels this polynomial (and every copy sharing its handle) and returns it
    Result<CoeffMultilinearPolynomial> relabel() {
        const int32_t rc = zk_cmle_relabel(context<F>(), h_->h);
        if (rc != ZK_OK) return rc;
        return *this;
    }
    // :272-282
    Result<CoeffMultilinearPolynomial> scalar_multiply(const Fe<F> &scalar) const {
        zk_cmle *o = nullptr;
        const int32_t rc = zk_cmle_scalar_multiply(context<F>(), h_->h, scalar.l.data(), &o);
        if (rc != ZK_OK) return rc;
        return CoeffMultilinearPolynomial(o);
    }
    // Add for & :350-373 (Err when an operand has fixed variables: relabel first)
    Result<CoeffMultilinearPolynomial> operator+(const CoeffMultilinearPolynomial &rhs) const {
        zk_cmle *o = nullptr;
        const int32_t rc = zk_cmle_add(context<F>(), h_->h, rhs.h_->h, &o);
        if (rc != ZK_OK) return rc;
        return CoeffMultilinearPolynomial(o);
    }
    // Mul for & :375-415 (this polynomial's variables first)
    Result<CoeffMultilinearPolynomial> operator*(const CoeffMultilinearPolynomial &rhs) const {
        zk_cmle *o = nullptr;
        const int32_t rc = zk_cmle_mul(context<F>(), h_->h, rhs.h_->h, &o);
        if (rc != ZK_OK) return rc;
        return CoeffMultilinearPolynomial(o);
    }
    zk_cmle *raw() const { return h_->h; }
};

template <class F>
class ProductPoly {
    std::vector<MultiLinearPolynomial<F>> polys_;
    explicit ProductPoly(std::vector<MultiLinearPolynomial<F>> p) : polys_(std::move(p)) {}
    std::vector<const zk_mle *> handles() const {
        std::vector<const zk_mle *> h;
        for (auto &p : polys_) h.push_back(p.raw());
        return h;
    }
    template <uint8_t, class> friend class SumcheckProver;
    template <class> friend class SumcheckVerifier;

public:
    // product_poly.rs:14-32
    static Result<ProductPoly> new_(std::vector<MultiLinearPolynomial<F>> polynomials) {
        std::vector<const zk_mle *> h;
        for (auto &p : polynomials) h.push_back(p.raw());
        const int32_t rc = zk_product_check(h.data(), h.size());
        if (rc != ZK_OK) return rc;
        return ProductPoly(std::move(polynomials));
    }
    size_t n_vars() const { return polys_[0].n_vars(); }   // :86
    const std::vector<MultiLinearPolynomial<F>> &polynomials() const { return polys_; }
    Result<Fe<F>> evaluate(const std::vector<Fe<F>> &assignments) const {   // :36-44
        Fe<F> out;
        auto h = handles();
        const int32_t rc = zk_product_evaluate(context<F>(), h.data(), h.size(), reinterpret_cast<const uint64_t *>(assignments.data()),
                                               assignments.size(), out.l.data());
        if (rc != ZK_OK) return rc;
        return out;
    }
    Result<ProductPoly> partial_evaluate(size_t initial_var, const std::vector<Fe<F>> &assignments) const {   // :48-63
        std::vector<MultiLinearPolynomial<F>> out;
        for (auto &p : polys_) {
            auto r = p.partial_evaluate(initial_var, assignments);
            if (r.is_err()) return Result<ProductPoly>(ZK_ERR_PANIC_INDEX);
            out.push_back(r.unwrap());
        }
        return ProductPoly(std::move(out));
    }
    std::vector<Fe<F>> prod_reduce() const {   // :66-74
        auto h = handles();
        zk_mle *o = nullptr;
        std::vector<Fe<F>> v((size_t)1 << n_vars());
        if (zk_prod_reduce(context<F>(), h.data(), h.size(), &o) == ZK_OK) {
            zk_mle_download(context<F>(), o, reinterpret_cast<uint64_t *>(v.data()));
            zk_mle_free(context<F>(), o);
        }
        return v;
    }
    std::vector<uint8_t> to_bytes() const {   // :77-83
        std::vector<uint8_t> out;
        for (auto &p : polys_) {
            auto b = p.to_bytes();
            out.insert(out.end(), b.begin(), b.end());
        }
        return out;
    }
};

template <class F>
struct SumcheckProof {   // sumcheck/src/lib.rs:8-11 (fields private in the reference)
    Fe<F> sum;
    std::vector<std::vector<Fe<F>>> round_polys;
};
template <class F>
struct SubClaim {   // sumcheck/src/lib.rs:17-20
    Fe<F> sum;
    std::vector<Fe<F>> challenges;
};

template <uint8_t MAX_VAR_DEGREE, class F>
class SumcheckProver {
    static Result<std::pair<SumcheckProof<F>, std::vector<Fe<F>>>> run(const ProductPoly<F> &poly, Fe<F> sum, int absorb) {
        const size_t n = poly.n_vars(), ns = (size_t)MAX_VAR_DEGREE + 1;
        std::vector<zk_mle *> h;
        for (auto &p : poly.polys_) h.push_back(p.raw());
        std::vector<uint64_t> rp(4 * n * ns + 4), ch(4 * n + 4);
        const int32_t rc = zk_sumcheck_prove(context<F>(), h.data(), h.size(), MAX_VAR_DEGREE, sum.l.data(), absorb, /*consume=*/0,
                                             rp.data(), ch.data());
        if (rc != ZK_OK) return rc;
        SumcheckProof<F> proof{sum, {}};
        std::vector<Fe<F>> challenges(n);
        for (size_t r = 0; r < n; ++r) {
            std::vector<Fe<F>> row(ns);
            for (size_t t = 0; t < ns; ++t)
                for (int i = 0; i < 4; ++i) row[t].l[i] = rp[4 * (r * ns + t) + i];
            proof.round_polys.push_back(row);
            for (int i = 0; i < 4; ++i) challenges[r].l[i] = ch[4 * r + i];
        }
        return std::make_pair(proof, challenges);
    }

public:
    static Result<SumcheckProof<F>> prove(const ProductPoly<F> &poly, Fe<F> sum) {   // prover.rs:15-20
        auto r = run(poly, sum, 1);
        if (r.is_err()) return Result<SumcheckProof<F>>(ZK_ERR_PANIC_INDEX);
        return r.unwrap().first;
    }
    static Result<std::pair<SumcheckProof<F>, std::vector<Fe<F>>>> prove_partial(const ProductPoly<F> &poly, Fe<F> sum) {   // :24-30
        return run(poly, sum, 0);
    }
    // polys.size() independent prove_partial calls (one ProductPoly each, same factor count and arity) proved side by side:
    // zk_sumcheck_prove_batch, one launch per round for all of them; element i equals prove_partial(polys[i], sums[i])
    static Result<std::vector<std::pair<SumcheckProof<F>, std::vector<Fe<F>>>>> prove_partial_batch(const std::vector<ProductPoly<F>> &polys,
                                                                                                  const std::vector<Fe<F>> &sums) {
        using Out = std::vector<std::pair<SumcheckProof<F>, std::vector<Fe<F>>>>;
        if (polys.size() != sums.size()) return Result<Out>(ZK_ERR_BAD_ARG);
        if (polys.empty()) return Out{};
        const size_t B = polys.size(), k = polys[0].polys_.size(), n = polys[0].n_vars(), ns = (size_t)MAX_VAR_DEGREE + 1;
        std::vector<zk_mle *> h;
        std::vector<uint64_t> s;
        for (size_t b = 0; b < B; ++b) {
            if (polys[b].polys_.size() != k) return Result<Out>(ZK_ERR_ARITY_MISMATCH);
            for (auto &p : polys[b].polys_) h.push_back(p.raw());
            s.insert(s.end(), sums[b].l.begin(), sums[b].l.end());
        }
        std::vector<uint64_t> rp(4 * B * n * ns + 4), ch(4 * B * n + 4);
        const int32_t rc = zk_sumcheck_prove_batch(context<F>(), B, h.data(), k, MAX_VAR_DEGREE, s.data(), /*consume=*/0, rp.data(), ch.data());
        if (rc != ZK_OK) return Result<Out>(rc);
        Out out;
        for (size_t b = 0; b < B; ++b) {
            SumcheckProof<F> proof{sums[b], {}};
            std::vector<Fe<F>> challenges(n);
            for (size_t r = 0; r < n; ++r) {
                std::vector<Fe<F>> row(ns);
                for (size_t t = 0; t < ns; ++t)
                    for (int i = 0; i < 4; ++i) row[t].l[i] = rp[4 * ((b * n + r) * ns + t) + i];
                proof.round_polys.push_back(row);
                for (int i = 0; i < 4; ++i) challenges[r].l[i] = ch[4 * (b * n + r) + i];
            }
            out.emplace_back(proof, challenges);
        }
        return out;
    }
};

template <class F>
class SumcheckVerifier {
    // round_polys is a Vec<Vec<F>>: every round goes to the library at its own length (verifier.rs:55-58)
    static std::vector<uint64_t> flatten(const SumcheckProof<F> &proof, std::vector<uint32_t> &lens) {
        std::vector<uint64_t> rp;
        lens.clear();
        for (auto &row : proof.round_polys) {
            lens.push_back((uint32_t)row.size());
            for (auto &e : row) rp.insert(rp.end(), e.l.begin(), e.l.end());
        }
        lens.push_back(0);
        rp.resize(rp.size() + 4);
        return rp;
    }

public:
    static Result<bool> verify(const ProductPoly<F> &poly, const SumcheckProof<F> &proof) {   // verifier.rs:15-33
        std::vector<uint32_t> lens;
        auto rp = flatten(proof, lens);
        auto h = poly.handles();
        int32_t ok = 0;
        const int32_t rc = zk_sumcheck_verify_lengths(context<F>(), h.data(), h.size(), proof.round_polys.size(), lens.data(),
                                                      proof.sum.l.data(), rp.data(), &ok);
        if (rc != ZK_OK) return rc;
        return ok != 0;
    }
    static Result<SubClaim<F>> verify_partial(const SumcheckProof<F> &proof) {   // verifier.rs:38-41
        std::vector<uint32_t> lens;
        auto rp = flatten(proof, lens);
        const size_t n = proof.round_polys.size();
        std::vector<uint64_t> ch(4 * n + 4);
        SubClaim<F> sub;
        const int32_t rc = zk_sumcheck_verify_partial_lengths(F::id, n, lens.data(), proof.sum.l.data(), rp.data(),
                                                              sub.sum.l.data(), ch.data());
        if (rc != ZK_OK) return rc;
        sub.challenges.resize(n);
        for (size_t r = 0; r < n; ++r)
            for (int i = 0; i < 4; ++i) sub.challenges[r].l[i] = ch[4 * r + i];
        return sub;
    }
};

class Transcript {   // transcript/src/lib.rs:5-35
    zk_transcript *t_ = nullptr;

public:
    Transcript() { zk_transcript_new(&t_); }
    ~Transcript() { zk_transcript_free(t_); }
    Transcript(const Transcript &) = delete;
    void append(const std::vector<uint8_t> &new_data) { zk_transcript_append(t_, new_data.data(), new_data.size()); }
    template <class F>
    Fe<F> sample_field_element() {
        Fe<F> e;
        zk_transcript_sample_field_element(t_, F::id, e.l.data());
        return e;
    }
    template <class F>
    std::vector<Fe<F>> sample_n_field_elements(size_t n) {
        std::vector<Fe<F>> v(n);   // transcript/src/lib.rs:32-34
        zk_transcript_sample_n_field_elements(t_, F::id, n, reinterpret_cast<uint64_t *>(v.data()));
        return v;
    }
};

// fft/src/lib.rs:4-19.  The reference panics on bad lengths; here that is a std::runtime_error carrying the message.
template <class F>
inline std::vector<Fe<F>> fft(const std::vector<Fe<F>> &coefficients) {
    std::vector<Fe<F>> out(coefficients.size());
    const int32_t rc = zk_fft_host(context<F>(), reinterpret_cast<const uint64_t *>(coefficients.data()), coefficients.size(),
                                   reinterpret_cast<uint64_t *>(out.data()));
    if (rc != ZK_OK) throw std::runtime_error(zk_strerror(rc));
    return out;
}
// fft/src/lib.rs:21-46 -- any omega; "values must be a power of 2" as the reference
template <class F>
inline std::vector<Fe<F>> fft_internal(const std::vector<Fe<F>> &values, const Fe<F> &omega) {
    std::vector<Fe<F>> out(values.size());
    const int32_t rc = zk_fft_internal_host(context<F>(), reinterpret_cast<const uint64_t *>(values.data()), values.size(), omega.l.data(),
                                            reinterpret_cast<uint64_t *>(out.data()));
    if (rc != ZK_OK) throw std::runtime_error(zk_strerror(rc));
    return out;
}
// polynomial/src/multilinear/pairing_index.rs:24-26: a bit sequence of n ones (mask(1) -> 1, mask(3) -> 0b111).  The reference
// overflows (panics in debug builds) at n >= usize::BITS; here that is the index panic status.
inline size_t mask(uint8_t n) {
    if (n >= sizeof(size_t) * 8) throw std::runtime_error(zk_strerror(ZK_ERR_PANIC_INDEX));
    return ((size_t)1 << n) - 1;
}
// polynomial/src/multilinear/pairing_index.rs:2-9 (host index arithmetic; the kernels compute the same indices inline)
inline std::vector<std::pair<size_t, size_t>> index_pair(uint8_t n_vars, uint8_t index) {
    if (n_vars == 0 || index > n_vars - 1) throw std::runtime_error(zk_strerror(ZK_ERR_PANIC_INDEX));
    const unsigned pos = n_vars - 1 - index;
    std::vector<std::pair<size_t, size_t>> out;
    for (size_t j = 0; j < ((size_t)1 << (n_vars - 1)); ++j) {
        const size_t left = ((j >> pos) << (pos + 1)) | (j & mask((uint8_t)pos));
        out.emplace_back(left, left | ((size_t)1 << pos));
    }
    return out;
}
template <class F>
inline std::vector<Fe<F>> ifft(const std::vector<Fe<F>> &evaluations) {
    std::vector<Fe<F>> out(evaluations.size());
    const int32_t rc = zk_ifft_host(context<F>(), reinterpret_cast<const uint64_t *>(evaluations.data()), evaluations.size(),
                                    reinterpret_cast<uint64_t *>(out.data()));
    if (rc != ZK_OK) throw std::runtime_error(zk_strerror(rc));
    return out;
}

// ---- GKR-shaped driver (the reference has no gkr crate; formats are this library's) ----------
// prove_partial (prover.rs:24-30) on a sum of products: terms[i] = the factors of product i.
template <class F>
struct TermsProof {
    std::vector<std::vector<Fe<F>>> round_polys;
    std::vector<Fe<F>> challenges, finals;   // finals: every factor at the challenge point, term after term
};
template <uint8_t MAX_VAR_DEGREE, class F>
inline Result<TermsProof<F>> prove_partial_terms(const std::vector<std::vector<MultiLinearPolynomial<F>>> &terms, Fe<F> sum) {
    std::vector<zk_mle *> h;
    std::vector<uint64_t> tk;
    for (auto &t : terms) {
        tk.push_back(t.size());
        for (auto &p : t) h.push_back(p.raw());
    }
    if (h.empty()) return Result<TermsProof<F>>(ZK_ERR_EMPTY_PRODUCT);
    const size_t n = terms[0][0].n_vars(), ns = (size_t)MAX_VAR_DEGREE + 1;
    std::vector<uint64_t> rp(4 * n * ns + 4), ch(4 * n + 4), fin(4 * h.size());
    const int32_t rc = zk_sumcheck_prove_terms(context<F>(), h.data(), tk.data(), tk.size(), MAX_VAR_DEGREE, sum.l.data(), 0,
                                               rp.data(), ch.data(), fin.data());
    if (rc != ZK_OK) return rc;
    TermsProof<F> out;
    out.challenges.resize(n);
    out.finals.resize(h.size());
    for (size_t r = 0; r < n; ++r) {
        std::vector<Fe<F>> row(ns);
        for (size_t t = 0; t < ns; ++t)
            for (int i = 0; i < 4; ++i) row[t].l[i] = rp[4 * (r * ns + t) + i];
        out.round_polys.push_back(row);
        for (int i = 0; i < 4; ++i) out.challenges[r].l[i] = ch[4 * r + i];
    }
    for (size_t f = 0; f < h.size(); ++f)
        for (int i = 0; i < 4; ++i) out.finals[f].l[i] = fin[4 * f + i];
    return out;
}

struct Layer {   // 2^log_out gates over 2^log_in values; op 0 = add, 1 = mul
    size_t log_out, log_in;
    std::vector<uint8_t> op;
    std::vector<uint32_t> left, right;
};
template <class F>
struct GkrProof {
    std::vector<Fe<F>> elements;   // per layer [round polys #1 | round polys #2 | W(u) | W(v)]
};
template <class F>
class Circuit {
    struct Handle {
        zk_circuit *h = nullptr;
        ~Handle() { if (h) zk_circuit_free(h); }
    };
    std::shared_ptr<Handle> h_;
    explicit Circuit(zk_circuit *h) : h_(std::make_shared<Handle>()) { h_->h = h; }

public:
    // layers[0] = output layer
    static Result<Circuit> new_(const std::vector<Layer> &layers) {
        zk_circuit *z = nullptr;
        int32_t rc = zk_circuit_create(context<F>(), &z);
        if (rc != ZK_OK) return rc;
        Circuit c(z);
        for (auto &l : layers) {
            if (l.op.size() != ((size_t)1 << l.log_out) || l.left.size() != l.op.size() || l.right.size() != l.op.size())
                return Result<Circuit>(ZK_ERR_BAD_ARG);
            rc = zk_circuit_add_layer(z, l.log_out, l.log_in, l.op.data(), l.left.data(), l.right.data());
            if (rc != ZK_OK) return rc;
        }
        return c;
    }
    Result<MultiLinearPolynomial<F>> evaluate(const MultiLinearPolynomial<F> &input) const {
        zk_mle *o = nullptr;
        const int32_t rc = zk_gkr_evaluate(h_->h, input.raw(), &o);
        if (rc != ZK_OK) return rc;
        return MultiLinearPolynomial<F>(o);
    }
    // -> (outputs, proof)
    Result<std::pair<MultiLinearPolynomial<F>, GkrProof<F>>> prove(const MultiLinearPolynomial<F> &input,
                                                                   const std::array<uint8_t, 32> &seed) const {
        uint64_t n = 0;
        zk_circuit_proof_elems(h_->h, &n);
        GkrProof<F> proof;
        proof.elements.resize(n);
        zk_mle *o = nullptr;
        const int32_t rc = zk_gkr_prove(h_->h, input.raw(), seed.data(), &o, reinterpret_cast<uint64_t *>(proof.elements.data()));
        if (rc != ZK_OK) return rc;
        return std::make_pair(MultiLinearPolynomial<F>(o), proof);
    }
    // Ok(true) accept, Ok(false) reject, Err on misuse
    Result<bool> verify(const MultiLinearPolynomial<F> &input, const MultiLinearPolynomial<F> &outputs,
                        const std::array<uint8_t, 32> &seed, const GkrProof<F> &proof) const {
        uint64_t n = 0;
        zk_circuit_proof_elems(h_->h, &n);
        if (proof.elements.size() != n) return Result<bool>(ZK_ERR_BAD_ARG);
        const int32_t rc = zk_gkr_verify(h_->h, input.raw(), outputs.raw(), seed.data(),
                                         reinterpret_cast<const uint64_t *>(proof.elements.data()));
        if (rc == ZK_OK) return true;
        if (rc == ZK_ERR_VERIFY_SUM || rc == ZK_ERR_GKR_REJECT) return false;
        return rc;
    }
};

}  // namespace zk
