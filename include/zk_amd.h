/*
 * zk_amd.h -- C ABI of libzk_amd.so: the MI355X (gfx950) implementation of the iammadab/zk sumcheck /
 * MLE-fold / NTT hot path.
 *
 * The reference has no FFI: its boundary for this path is the public Rust API of the
 * `polynomial`, `sumcheck`, `transcript` and `fft` crates.  Each entry point below names the reference item it
 * replaces (file:line relative to the reference checkout); bindings/rust/ shows the shim that maps the
 * reference's type and method names onto these calls, INTEGRATION.md shows how a maintainer wires it in.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.  Every call returns int32_t: 0 = ok, negative =
 *    zk_status.  zk_strerror() returns the reference's own `Err(&'static str)` text where one exists.
 *    No exception or panic crosses the boundary: misuse the reference panics on returns ZK_ERR_PANIC_*.
 *  - Field elements cross as `const uint64_t*`: ark-ff 0.5.0 `Fp<MontBackend<_,4>>` in memory -- 4 little-endian
 *    u64 limbs, Montgomery form (R = 2^256), fully reduced.  A `Vec<F>` is passed as-is, no conversion.
 *  - Device memory lives behind opaque handles (zk_mle).  The `*_host` calls are the value-semantics
 *    convenience forms (upload, compute, download) matching the reference's Vec-in / Vec-out signatures.
 *  - A zk_ctx owns one device, one HIP stream and its scratch; it is not thread-safe, distinct contexts are
 *    independent.  All work is stream-ordered; calls that return host data synchronise that stream.
 *  - There is NO CPU fallback: without a usable gfx950 device zk_ctx_create fails with ZK_ERR_NO_DEVICE.
 */
#ifndef ZK_AMD_H
#define ZK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_AMD_ABI_VERSION 6   /* 3: + zk_comm (RCCL / host), zk_shard_prover_run, zk_ntt_sharded, sample_n, zk_ctx_trim, zk_mle_equal
                                  4: + zk_sumcheck_verify_lengths / _verify_partial_lengths (per-round degrees, verifier.rs:55-58)
                                  5: + zk_comm_info, zk_bench_evaluate_device
                                  6: + zk_sumcheck_prove_batch, zk_batch_last_stats */

typedef enum zk_field {
    ZK_FIELD_BN254_FR = 0,     /* north-star field (not a dependency of the reference: SURVEY D2) */
    ZK_FIELD_BLS12_381_FR = 1, /* field of the reference's polynomial/sumcheck tests */
    ZK_FIELD_BLS12_377_FR = 2  /* field of the reference's fft test */
} zk_field;

typedef enum zk_status {
    ZK_OK = 0,
    ZK_ERR_EVAL_LEN = -1,       /* "evaluation vec len should equal 2^n_vars"            evaluation_form.rs:20 */
    ZK_ERR_EVAL_ARITY = -2,     /* "evaluate must assign to all variables"               evaluation_form.rs:85 */
    ZK_ERR_EMPTY_PRODUCT = -3,  /* "cannot create product polynomial from empty ..."     product_poly.rs:16    */
    ZK_ERR_ARITY_MISMATCH = -4, /* "... don't share the same number of variables"        product_poly.rs:25    */
    ZK_ERR_PANIC_INDEX = -5,    /* reference panics: integer underflow in index_pair / slice (evaluation_form.rs:55,75) */
    ZK_ERR_FFT_NOT_POW2 = -6,   /* reference panics: "values must be a power of 2"       fft/src/lib.rs:29     */
    ZK_ERR_FFT_NO_ROOT = -7,    /* reference panics: get_root_of_unity(..).unwrap()      fft/src/lib.rs:6,14   */
    ZK_ERR_VERIFY_ROUNDS = -8,  /* "invalid proof: require 1 round poly for each variable in poly" verifier.rs:18 */
    ZK_ERR_VERIFY_SUM = -9,     /* "verifier check failed: claimed_sum != p(0) + p(1)"   verifier.rs:64        */
    ZK_ERR_COEFF_RANGE = -10,   /* "coefficient map represents more than specificed number of variables" coefficient_form.rs:184 */
    ZK_ERR_PANIC_INVERSE = -11, /* reference panics: (x_i - x_j).inverse().unwrap() on a repeated x  univariate_poly.rs:68 */
    ZK_ERR_EVAL_ASSIGNMENT = -12, /* "evaluate requires an assignment for every variable"  coefficient_form.rs:48 */
    ZK_ERR_SELECTOR_LEN = -13,    /* "the selector array len should be the same as the number of variables" coefficient_form.rs:290 */
    ZK_ERR_SELECTOR_SINGLE = -14, /* "only select single variable, cannot get indexes for constant or multiple variables" :303 */
    ZK_ERR_BAD_ARG = -20,
    ZK_ERR_BAD_FIELD = -21,
    ZK_ERR_NO_DEVICE = -22,     /* no gfx950 device / HIP runtime failure at context creation */
    ZK_ERR_HIP = -23,           /* a HIP call failed; zk_last_hip_error() has the text */
    ZK_ERR_ALLOC = -24,
    ZK_ERR_UNSUPPORTED = -25,
    ZK_ERR_CONTEXT_MISMATCH = -26,
    ZK_ERR_GKR_REJECT = -27,    /* GKR-shaped driver: a layer's wiring check or the input-layer check failed (no reference text) */
    ZK_ERR_COMM = -28           /* a collective failed (RCCL error text in zk_last_hip_error) or librccl could not be loaded */
} zk_status;

typedef struct zk_ctx zk_ctx;               /* one device + stream + scratch */
typedef struct zk_mle zk_mle;               /* device-resident table of 2^n_vars elements */
typedef struct zk_transcript zk_transcript; /* host-side Keccak-256 Fiat-Shamir sponge */
typedef struct zk_upoly zk_upoly;           /* device-resident coefficient vector of any length (0 included) */
typedef struct zk_cmle zk_cmle;             /* device-resident dense CoeffMultilinearPolynomial: the coefficients of its present keys, key order */

/* ---- library ---------------------------------------------------------------------------------------- */
int32_t zk_abi_version(void);
const char *zk_strerror(int32_t status);
const char *zk_last_hip_error(void);
int32_t zk_device_count(int32_t *out_count);

/* ---- context ---------------------------------------------------------------------------------------- */
int32_t zk_ctx_create(int32_t field, int32_t device, zk_ctx **out_ctx);
int32_t zk_ctx_destroy(zk_ctx *ctx);
int32_t zk_ctx_synchronize(zk_ctx *ctx);
/* run on a caller-owned hipStream_t (e.g. torch's current stream; NULL = the legacy default stream) instead of the
 * context's own non-blocking stream; zk_ctx_use_own_stream switches back.  Both synchronise the stream being left. */
int32_t zk_ctx_set_stream(zk_ctx *ctx, void *hip_stream);
int32_t zk_ctx_use_own_stream(zk_ctx *ctx);
int32_t zk_ctx_field(const zk_ctx *ctx, int32_t *out_field);
/* freed tables are kept in a per-context pool (hipMalloc/hipFree of a 512 MiB block costs more than a 2^24 fold); the pool
 * is trimmed automatically when it exceeds half of the device's free memory or an allocation fails; this drops it now. */
int32_t zk_ctx_trim(zk_ctx *ctx);
/* modulus as 4 LE limbs; two-adicity s of p-1 */
int32_t zk_field_modulus(int32_t field, uint64_t out_p[4]);
int32_t zk_field_two_adicity(int32_t field, int32_t *out_s);
/* host-side element helpers for callers without ark-ff (tests, Python): F::from(u64), into_bigint, from_be_bytes_mod_order */
/* F::get_root_of_unity(2^log_n) (fft/src/lib.rs:6,14): g^((p-1)/2^log_n); None -> ZK_ERR_FFT_NO_ROOT */
int32_t zk_field_root_of_unity(int32_t field, uint64_t log_n, uint64_t out[4]);
int32_t zk_fe_from_u64(int32_t field, uint64_t v, uint64_t out[4]);
int32_t zk_fe_from_canonical(int32_t field, const uint64_t limbs[4], uint64_t out[4]);
int32_t zk_fe_to_canonical(int32_t field, const uint64_t a[4], uint64_t out_limbs[4]);
int32_t zk_fe_from_be_bytes_mod_order(int32_t field, const uint8_t *bytes, size_t len, uint64_t out[4]);

/* ---- MultiLinearPolynomial  (polynomial/src/multilinear/evaluation_form.rs) ------------------------------- */
/* ::new(n_vars, evaluations) :15-27 -- len != 2^n_vars -> ZK_ERR_EVAL_LEN.  Copies host -> device. */
int32_t zk_mle_upload(zk_ctx *ctx, uint64_t n_vars, const uint64_t *evals, uint64_t len, zk_mle **out);
/* uninitialised table (for outputs) / synthetic table (bench inputs: SURVEY 8d generator, element i of stream `seed`) */
int32_t zk_mle_alloc(zk_ctx *ctx, uint64_t n_vars, zk_mle **out);
int32_t zk_mle_fill_random(zk_ctx *ctx, zk_mle *t, uint64_t seed, uint64_t first_index);
int32_t zk_mle_clone(zk_ctx *ctx, const zk_mle *t, zk_mle **out);                    /* #[derive(Clone)] :4 */
int32_t zk_mle_free(zk_ctx *ctx, zk_mle *t);
int32_t zk_mle_n_vars(const zk_mle *t, uint64_t *out_n_vars);                         /* ::n_vars :30 */
int32_t zk_mle_download(zk_ctx *ctx, const zk_mle *t, uint64_t *out_evals);           /* ::evaluation_slice :92 */
int32_t zk_mle_device_ptr(const zk_mle *t, void **out_ptr);                           /* raw device pointer (interop) */
/* #[derive(PartialEq)] :4 -- n_vars and every evaluation equal (compared on the device; canonical representation) */
int32_t zk_mle_equal(zk_ctx *ctx, const zk_mle *a, const zk_mle *b, int32_t *out_equal);
/* ::partial_evaluate(initial_var, assignments) :40-80 -> new table of n_vars - n_assign variables */
int32_t zk_mle_partial_evaluate(zk_ctx *ctx, const zk_mle *t, uint64_t initial_var,
                                const uint64_t *assignments, uint64_t n_assign, zk_mle **out);
/* the sumcheck fold: partial_evaluate(0, [r]) written into a preallocated (n_vars-1)-variable table (no allocation) */
int32_t zk_mle_fold_into(zk_ctx *ctx, const zk_mle *t, const uint64_t r[4], zk_mle *out);
/* ::evaluate(assignments) :83-89 -- n_point != n_vars -> ZK_ERR_EVAL_ARITY */
int32_t zk_mle_evaluate(zk_ctx *ctx, const zk_mle *t, const uint64_t *point, uint64_t n_point, uint64_t out[4]);
/* ::to_bytes :97-103 -- 32-byte big-endian canonical integers, concatenated (32 << n_vars bytes) */
int32_t zk_mle_to_bytes(zk_ctx *ctx, const zk_mle *t, uint8_t *out_bytes);
/* value-semantics forms of the two calls above the reference's own tests use */
int32_t zk_mle_partial_evaluate_host(zk_ctx *ctx, uint64_t n_vars, const uint64_t *evals, uint64_t len,
                                     uint64_t initial_var, const uint64_t *assignments, uint64_t n_assign,
                                     uint64_t *out_evals /* 2^(n_vars-n_assign) elements */);

/* ---- the step before the path: CoeffMultilinearPolynomial::to_evaluation_form (coefficient_form.rs:340-347) ------------
 * Sparse coefficient form {key -> coefficient} (key bit v <-> variable v, selector_to_index :418-430; the BTreeMap of
 * coefficient_form.rs:27-30 passed as parallel arrays, duplicate keys are summed like ::new :164-171) -> the dense
 * evaluation table in hypercube order, resident on the device.  key >= 2^n_vars -> ZK_ERR_COEFF_RANGE (:183-186).
 * n_vars == 0 -> ZK_ERR_EVAL_LEN (the reference returns an empty vector there, which cannot be a table). */
int32_t zk_coeff_to_evaluation(zk_ctx *ctx, uint64_t n_vars, const uint64_t *keys, const uint64_t *coeffs, uint64_t n_terms,
                               zk_mle **out);

/* ---- ProductPoly  (polynomial/src/product_poly.rs) ---------------------------------------------------------- */
/* ::new :14-32 -- k == 0 -> ZK_ERR_EMPTY_PRODUCT, unequal arity -> ZK_ERR_ARITY_MISMATCH.  Validation only:
 * a product is passed to the calls below as an array of k table handles. */
int32_t zk_product_check(const zk_mle *const *factors, uint64_t k);
/* ::prod_reduce :66-74 -> new table, element-wise product of the k factors */
int32_t zk_prod_reduce(zk_ctx *ctx, const zk_mle *const *factors, uint64_t k, zk_mle **out);
/* ::evaluate :36-44 */
int32_t zk_product_evaluate(zk_ctx *ctx, const zk_mle *const *factors, uint64_t k, const uint64_t *point,
                            uint64_t n_point, uint64_t out[4]);
/* one prover round's polynomial in evaluation form (sumcheck/src/prover.rs:49-56):
 * out[t] = sum_x prod_f P_f(t, x), t = 0..max_var_degree -- (max_var_degree+1) elements */
int32_t zk_round_sums(zk_ctx *ctx, const zk_mle *const *factors, uint64_t k, uint32_t max_var_degree,
                      uint64_t *out_sums);

/* ---- Transcript  (transcript/src/lib.rs) -- host side ------------------------------------------------------- */
int32_t zk_transcript_new(zk_transcript **out);                                        /* ::new :10-14 */
int32_t zk_transcript_free(zk_transcript *t);
int32_t zk_transcript_append(zk_transcript *t, const uint8_t *data, size_t len);       /* ::append :16-18 */
int32_t zk_transcript_sample_field_element(zk_transcript *t, int32_t field, uint64_t out[4]); /* :27-30 */
int32_t zk_transcript_sample_n_field_elements(zk_transcript *t, int32_t field, uint64_t n, uint64_t *out); /* :32-34, n*4 u64 */
int32_t zk_transcript_sample_challenge(zk_transcript *t, uint8_t out[32]);             /* :20-25 (private in the reference) */
int32_t zk_keccak256(const uint8_t *data, size_t len, uint8_t out[32]);

/* ---- SumcheckProver<MAX_VAR_DEGREE, F>  (sumcheck/src/prover.rs) ---------------------------------------------- */
/* ::prove :15-20 (absorb_table != 0: the whole table is serialised and absorbed first) and ::prove_partial :24-30
 * (absorb_table == 0).  The factor tables are consumed as scratch only if `consume` != 0 (the reference takes the
 * polynomial by value); otherwise they are left intact.
 * out_round_polys: n_vars * (max_var_degree+1) elements (SumcheckProof.round_polys, row-major);
 * out_challenges: n_vars elements (the Vec<F> prove_partial returns). */
int32_t zk_sumcheck_prove(zk_ctx *ctx, zk_mle *const *factors, uint64_t k, uint32_t max_var_degree,
                          const uint64_t sum[4], int32_t absorb_table, int32_t consume,
                          uint64_t *out_round_polys, uint64_t *out_challenges);
/* n_proofs INDEPENDENT ::prove_partial calls (prover.rs:24-30: one per ProductPoly; the reference's callers -- a GKR prover's layers,
 * SURVEY 8d config 4 -- simply call it n_proofs times) of ONE shape (k factors, max_var_degree) and ONE size, proved side by side:
 * each proof keeps its own transcript and is bit-identical to what zk_sumcheck_prove(absorb_table = 0) returns for the same inputs,
 * but every round of all proofs is ONE kernel launch (up to 8 proofs per launch; larger batches run in groups), so the per-round
 * latency chain is paid once per group instead of once per proof.
 * factors: n_proofs * k handles, proof after proof; sums: n_proofs * 4 u64; out_round_polys: n_proofs * n_vars * (max_var_degree+1)
 * elements; out_challenges: n_proofs * n_vars elements (proof-major).  consume as in zk_sumcheck_prove (a handle listed twice
 * anywhere in the batch is proved out of place).  Errors: those of zk_sumcheck_prove; proofs of different n_vars ->
 * ZK_ERR_ARITY_MISMATCH. */
int32_t zk_sumcheck_prove_batch(zk_ctx *ctx, uint64_t n_proofs, zk_mle *const *factors, uint64_t k, uint32_t max_var_degree,
                                const uint64_t *sums, int32_t consume, uint64_t *out_round_polys, uint64_t *out_challenges);
/* what the calling thread's last zk_sumcheck_prove_batch did: launches issued once for all proofs of a group (merged) / launches
 * issued proof by proof because the kernel has no batched form for that shape (replayed).  Diagnostics only. */
int32_t zk_batch_last_stats(uint64_t *out_merged, uint64_t *out_replayed);
/* value-semantics form: k host tables of 2^n_vars elements each */
int32_t zk_sumcheck_prove_host(zk_ctx *ctx, const uint64_t *const *tables, uint64_t k, uint64_t n_vars,
                               uint32_t max_var_degree, const uint64_t sum[4], int32_t absorb_table,
                               uint64_t *out_round_polys, uint64_t *out_challenges);

/* Stepwise form of the same loop for a table sharded across devices.  Rank g of `world` (a power of
 * two) holds the shard {idx : idx mod world == g} as an (n - log2 world)-variable table with local index idx / world,
 * so every pair (j, j + 2^(m-1)) of the first n - log2 world rounds is local.  Every rank calls these in lockstep on
 * its own context; everything is asynchronous on the context's stream (use zk_ctx_set_stream to share the stream the
 * collective runs on):
 *   round_begin : (fold at the previous challenge +) local round sums -> digit lanes: per element 8 uint64 lanes, lane i
 *                 = 32-bit digit i of the Montgomery representative, zero-extended.  The caller all-reduces (sum) the
 *                 (D+1)*8 lanes across ranks -- the ONE collective of the round; integer lane sums of <= 2^16 ranks
 *                 cannot overflow and carry exactly the field sum (RCCL has no mod-p reduction).
 *   round_finish: carry-propagate + reduce the summed lanes mod p, absorb the round polynomial, squeeze the challenge
 *                 (identical on every rank: same transcript, same bytes).
 * At any point after a round_finish (typically once the local tables are <= 2^10 elements, and at the latest after the
 * last local round): tail_ptr applies the pending challenge and exposes this rank's k shard tables as one device buffer
 * [k][2^s]; the caller all-gathers them rank-major into [world][k][2^s] and tail_rounds rebuilds the (s + log2 world)-
 * variable tables and runs ALL remaining rounds on every rank redundantly -- no further collective.
 * results downloads the proof (total_rounds = n rounds).  `sum` is the GLOBAL claimed sum (prover.rs:42). */
typedef struct zk_shard_prover zk_shard_prover;
int32_t zk_shard_prover_create(zk_ctx *ctx, zk_mle *const *factors, uint64_t k, uint32_t max_var_degree,
                               const uint64_t sum[4], uint32_t world, zk_shard_prover **out);
int32_t zk_shard_prover_destroy(zk_shard_prover *sp);
int32_t zk_shard_prover_rounds(zk_shard_prover *sp, uint64_t *out_local, uint64_t *out_total, uint64_t *out_done);
int32_t zk_shard_prover_lanes_ptr(zk_shard_prover *sp, void **out_device_ptr, uint64_t *out_n_lanes);
int32_t zk_shard_prover_round_begin(zk_shard_prover *sp);
int32_t zk_shard_prover_round_finish(zk_shard_prover *sp);
int32_t zk_shard_prover_tail_ptr(zk_shard_prover *sp, void **out_device_ptr, uint64_t *out_n_elems);
int32_t zk_shard_prover_tail_rounds(zk_shard_prover *sp, const void *gathered_device /* [world][k][2^s] elements */);
int32_t zk_shard_prover_results(zk_shard_prover *sp, uint64_t *out_round_polys, uint64_t *out_challenges);
/* ---- communicator: the exchange steps of the sharded paths, driven from inside the library --------------------------
 * One zk_comm per rank (= per process = per GPU).  Two kinds:
 *   RCCL (the product path, xGMI): zk_comm_unique_id on one rank, the 128 bytes distributed by the host's own means (the
 *     Rust side: any channel it already has; Python: torch.distributed), then zk_comm_create_rccl on every rank
 *     (ncclCommInitRank); or zk_comm_wrap_rccl around a ncclComm_t the host already owns.  librccl.so.1 is dlopen'ed on
 *     first use, so single-GPU users never load it.  Collectives are enqueued on the context's stream: no host waits.
 *   host callbacks (tests / hosts with their own transport): the library stages the buffer through pinned memory,
 *     synchronises, and calls back; the callbacks return 0 on success.  Same control flow, different transport.
 *       allreduce(user, buf, n)               : buf[i] <- sum over ranks of buf[i], n uint64 lanes (cannot overflow)
 *       allgather(user, send, n, recv)        : recv[r*n .. r*n+n) <- rank r's send
 *       alltoall (user, send, recv, n)        : recv[r*n .. ) <- rank r's send[me*n .. ), n uint64 per peer */
typedef struct zk_comm zk_comm;
typedef int32_t (*zk_host_allreduce_fn)(void *user, uint64_t *buf, uint64_t n);
typedef int32_t (*zk_host_allgather_fn)(void *user, const uint64_t *send, uint64_t n, uint64_t *recv);
typedef int32_t (*zk_host_alltoall_fn)(void *user, const uint64_t *send, uint64_t *recv, uint64_t n_per_peer);
int32_t zk_comm_unique_id(uint8_t out_id[128]);
int32_t zk_comm_create_rccl(zk_ctx *ctx, const uint8_t id[128], uint32_t world, uint32_t rank, zk_comm **out);
int32_t zk_comm_wrap_rccl(zk_ctx *ctx, void *nccl_comm, uint32_t world, uint32_t rank, zk_comm **out);
int32_t zk_comm_create_host(zk_ctx *ctx, uint32_t world, uint32_t rank, zk_host_allreduce_fn allreduce,
                            zk_host_allgather_fn allgather, zk_host_alltoall_fn alltoall, void *user, zk_comm **out);
int32_t zk_comm_destroy(zk_comm *comm);
/* what the transport itself reports: RCCL's version (ncclGetVersion; 0 for the host transport) and the communicator's own rank
 * count and rank (ncclCommCount / ncclCommUserRank).  Any out pointer may be NULL. */
int32_t zk_comm_info(zk_comm *comm, int32_t *out_rccl_version, uint32_t *out_ranks, uint32_t *out_rank);
/* The WHOLE sharded prover (prove_partial, sumcheck/src/prover.rs:24-30,44-68) on a freshly created zk_shard_prover:
 * per local round {round_begin -> all-reduce of the (D+1)*8 lanes -> round_finish} while more than `gather_below` local
 * variables remain, then tail_ptr -> all-gather -> tail_rounds.  With an RCCL comm everything is enqueued on the context's
 * stream with ZERO host synchronisations (the all-reduce is the round's one collective); fetch the proof with
 * zk_shard_prover_results.  Every rank calls it with the same arguments. */
int32_t zk_shard_prover_run(zk_shard_prover *sp, zk_comm *comm, uint32_t gather_below);
/* The same run with a breakdown by HIP events on the stream (each record stalls the stream a few microseconds: a breakdown,
 * not a timing): out_ms[0] local kernels of the exchanging rounds, [1] the per-round all-reduces, [2] the all-gather of the
 * shard tails (with the pending fold), [3] the replicated tail rounds.  Synchronises. */
int32_t zk_shard_prover_run_phases(zk_shard_prover *sp, zk_comm *comm, uint32_t gather_below, double out_ms[4]);
/* Failure rule of the two collective entry points (zk_shard_prover_run*, zk_ntt_sharded): a rank whose local step fails
 * between collectives aborts a communicator it created (ncclCommAbort, so its peers' pending collectives return an error
 * instead of hanging) and returns the error; the zk_comm is dead afterwards -- every later call on it returns ZK_ERR_COMM --
 * and must be destroyed.  A wrapped communicator (zk_comm_wrap_rccl) is only marked dead: aborting it is its owner's call. */
/* fft / ifft (fft/src/lib.rs:4-19) of an N = world * 2^m point vector held as index-mod-world shards ("strided": rank r
 * holds x[r + world*j]); ONE all-to-all.  forward: strided in -> "sliced" out (rank s holds X[k], k mod M in its slice of
 * M / world, as world rows of M / world); inverse: sliced in -> strided out, scaled 1/N.  shard is not modified;
 * out != shard, same size.  m >= log2 world.  Asynchronous with an RCCL comm. */
int32_t zk_ntt_sharded(zk_ctx *ctx, zk_comm *comm, const zk_mle *shard, int32_t inverse, zk_mle *out);

/* ---- sharding by index mod world: the layout of zk_shard_prover_create and zk_ntt_sharded's strided input -------------
 * (no reference item: the reference is single-process and hands over one natural-order Vec<F>, evaluation_form.rs:15).
 * The kernels are permutations (no field arithmetic): bit-exact.  Symbols only; the ABI version is unchanged. */
/* shard rank of a natural-order table: {idx : idx mod world == rank}, local index idx / world (the layout of
   zk_shard_prover_create and zk_ntt_sharded's strided input); n_vars/len are the FULL table's; world a power of two,
   1 <= world <= min(2^n_vars, 2^16); the host array is not needed after return */
int32_t zk_mle_upload_shard(zk_ctx *ctx, uint64_t n_vars, const uint64_t *evals, uint64_t len,
                            uint32_t world, uint32_t rank, zk_mle **out);
/* all world shards of a resident table in one pass (out_shards[world]); t is unchanged; asynchronous
   (world > 64: the shards' pointer table is staged through the host first, one wait for the stream) */
int32_t zk_mle_split(zk_ctx *ctx, const zk_mle *t, uint32_t world, zk_mle **out_shards);
/* inverse of zk_mle_split: world equal-size shards -> the natural-order table; asynchronous (world > 64: as zk_mle_split) */
int32_t zk_mle_interleave(zk_ctx *ctx, const zk_mle *const *shards, uint32_t world, zk_mle **out);
/* every rank: all-gather of the shards over comm + interleave -> the natural-order table on every rank.
   Asynchronous with an RCCL comm; same failure rule as zk_shard_prover_run / zk_ntt_sharded. */
int32_t zk_mle_unshard(zk_ctx *ctx, zk_comm *comm, const zk_mle *shard, zk_mle **out);
/* Errors of the four: len != 2^n_vars -> ZK_ERR_EVAL_LEN; world 0, not a power of two, > 2^n_vars or > 2^16, rank >= world,
   null pointers -> ZK_ERR_BAD_ARG; shards of different sizes -> ZK_ERR_ARITY_MISMATCH; a handle of another context ->
   ZK_ERR_CONTEXT_MISMATCH; a dead comm -> ZK_ERR_COMM.  On an error nothing is allocated. */

/* raw device buffers on the context (pooled) and synchronous copies: for hosts that drive the exchange themselves */
int32_t zk_ctx_device_alloc(zk_ctx *ctx, uint64_t bytes, void **out_device_ptr);
int32_t zk_ctx_device_free(zk_ctx *ctx, void *device_ptr, uint64_t bytes);
int32_t zk_ctx_memcpy_dtoh(zk_ctx *ctx, void *dst_host, const void *src_device, uint64_t bytes);
int32_t zk_ctx_memcpy_htod(zk_ctx *ctx, void *dst_device, const void *src_host, uint64_t bytes);

/* ---- sum of products + GKR-shaped driver (NO reference crate; formats are this library's) ----
 * The reference's building block for GKR is prove_partial / verify_partial (sumcheck/src/prover.rs:24-30,
 * sumcheck/src/verifier.rs:38-41; intent: polynomial/src/multilinear/evaluation_form.rs:45-48).  A GKR layer polynomial is a
 * SUM of products of MLEs, so prove_partial is offered on sum_i prod_{f in term i} T_f: factors listed flat, term after
 * term, term_k[i] factors in term i (each <= max_var_degree, <= 4 terms, <= 8 factors in all, no table listed twice).
 * Round polynomials, transcript and challenges are exactly prove_partial's (one term == zk_sumcheck_prove with
 * absorb_table = 0).  out_final (optional, k*4 u64): every factor evaluated at the challenge point, i.e. the fold after
 * the last round that the reference computes and drops (prover.rs:64). */
int32_t zk_sumcheck_prove_terms(zk_ctx *ctx, zk_mle *const *factors, const uint64_t *term_k, uint64_t n_terms,
                                uint32_t max_var_degree, const uint64_t sum[4], int32_t consume,
                                uint64_t *out_round_polys, uint64_t *out_challenges, uint64_t *out_final);
/* eq(point, .) as a table: out[idx] = prod_v (bit_v(idx) ? point[v] : 1 - point[v]), variable 0 = index MSB */
int32_t zk_eq_table(zk_ctx *ctx, const uint64_t *point, uint64_t n_vars, zk_mle **out);

/* Layered arithmetic circuit, fan-in 2.  Layers are appended from the OUTPUT layer (0) towards the inputs; layer i has
 * 2^log_out gates over the 2^log_in values of layer i+1 (log_in of layer i == log_out of layer i+1; the last layer reads the
 * input table).  Gate z = (op[z], left[z], right[z]), op 0 = add, 1 = mul; indices follow the MLE convention
 * (variable 0 = index MSB).  1 <= log_in <= 30. */
typedef struct zk_circuit zk_circuit;
int32_t zk_circuit_create(zk_ctx *ctx, zk_circuit **out);
int32_t zk_circuit_add_layer(zk_circuit *c, uint64_t log_out, uint64_t log_in, const uint8_t *op, const uint32_t *left,
                             const uint32_t *right);
int32_t zk_circuit_free(zk_circuit *c);
int32_t zk_circuit_depth(const zk_circuit *c, uint64_t *out);
int32_t zk_circuit_layer_dims(const zk_circuit *c, uint64_t layer, uint64_t *out_log_out, uint64_t *out_log_in);
int32_t zk_circuit_proof_elems(const zk_circuit *c, uint64_t *out);   /* sum over layers of 6*log_in + 2 */
/* evaluate the circuit on the device: new table of 2^log_out(0) outputs */
int32_t zk_gkr_evaluate(const zk_circuit *c, const zk_mle *input, zk_mle **out_outputs);
/* GKR prover: per layer two prove_partial-style sumchecks (Libra's phase 1 over x, phase 2 over y), chained by their
 * sub-claims, on ONE transcript (Transcript semantics of transcript/src/lib.rs) that first absorbs seed (32 bytes: the caller's
 * domain separator / session id) and the library's own digests of the circuit, the inputs and the outputs (Keccak-256 tree
 * hash) -- the statement is bound before the output point is drawn.  out_proof: zk_circuit_proof_elems
 * elements, per layer [round polys #1 (log_in*3) | round polys #2 (log_in*3) | W(u) | W(v)].  Returns the outputs table. */
int32_t zk_gkr_prove(const zk_circuit *c, const zk_mle *input, const uint8_t seed[32], zk_mle **out_outputs,
                     uint64_t *out_proof);
/* ZK_OK = accept; ZK_ERR_VERIFY_SUM = a sumcheck round check failed; ZK_ERR_GKR_REJECT = wiring / input check failed.
 * The round checks of all layers are made first (host, while the device sums the wiring predicates), the wiring checks after
 * them: a proof with defects of both kinds reports the round check. */
int32_t zk_gkr_verify(const zk_circuit *c, const zk_mle *input, const zk_mle *outputs, const uint8_t seed[32],
                      const uint64_t *proof);

/* ---- pieces of the multi-GPU four-step NTT (orchestration: zk_amd/distributed.py ShardedNtt) -------------
 * The fft crate's transform (fft/src/lib.rs:21-46) over a vector sharded by index mod W: local zk_ntt per rank, then
 * the inter-rank twiddles, one all-to-all, and W-point transforms across the ranks' rows. */
/* t[j] *= scale * base^j */
int32_t zk_mle_mul_powers(zk_ctx *ctx, zk_mle *table, const uint64_t base[4], const uint64_t scale[4]);
/* in / out read as W = 2^log_w rows of L elements: out[k][j] = sum_r w^(r*k) in[r][j], w = get_root_of_unity(W)
 * (its inverse, unscaled, when inverse != 0); log_w <= 10 */
int32_t zk_dft_across(zk_ctx *ctx, const zk_mle *in, zk_mle *out, uint64_t log_w, int32_t inverse);

/* ---- SumcheckVerifier  (sumcheck/src/verifier.rs) -- host-side protocol logic; oracle check on device ------------ */
/* ::verify_partial :38-41 -> SubClaim{sum, challenges} */
int32_t zk_sumcheck_verify_partial(int32_t field, uint64_t n_rounds, uint32_t max_var_degree,
                                   const uint64_t sum[4], const uint64_t *round_polys,
                                   uint64_t out_subclaim_sum[4], uint64_t *out_challenges);
/* ::verify :15-33 -> *out_ok = 1 for Ok(true), 0 for Ok(false); Err -> negative status */
int32_t zk_sumcheck_verify(zk_ctx *ctx, const zk_mle *const *factors, uint64_t k, uint64_t n_round_polys,
                           uint32_t max_var_degree, const uint64_t sum[4], const uint64_t *round_polys,
                           int32_t *out_ok);

/* The same two with every round polynomial at ITS OWN length: SumcheckProof.round_polys is a Vec<Vec<F>> and
 * verify_internal hands each round to UnivariatePolynomial::interpolate as it comes (verifier.rs:55-58,
 * univariate_poly.rs:43-49), so a proof whose rounds carry different numbers of evaluations is legal input.
 * evals_per_round[r] (<= 256; 0 = the zero polynomial, 1 = a constant) evaluations for round r, stored back to back in
 * round_polys (sum of evals_per_round elements). */
int32_t zk_sumcheck_verify_partial_lengths(int32_t field, uint64_t n_rounds, const uint32_t *evals_per_round,
                                           const uint64_t sum[4], const uint64_t *round_polys,
                                           uint64_t out_subclaim_sum[4], uint64_t *out_challenges);
int32_t zk_sumcheck_verify_lengths(zk_ctx *ctx, const zk_mle *const *factors, uint64_t k, uint64_t n_round_polys,
                                   const uint32_t *evals_per_round, const uint64_t sum[4], const uint64_t *round_polys,
                                   int32_t *out_ok);

/* ---- fft crate  (fft/src/lib.rs) ------------------------------------------------------------------------------ */
/* fft :4-8 / ifft :11-19 on a device vector of 2^log_n elements (zk_mle doubles as the vector handle);
 * natural order in, natural order out, omega = F::get_root_of_unity(n). */
int32_t zk_ntt(zk_ctx *ctx, const zk_mle *in, int32_t inverse, zk_mle *out);
/* value-semantics forms: fft(Vec<F>) -> Vec<F>; n == 0 or n > 2^two_adicity -> ZK_ERR_FFT_NO_ROOT,
 * n not a power of two -> ZK_ERR_FFT_NO_ROOT (get_root_of_unity returns None first, fft/src/lib.rs:6) */
int32_t zk_fft_host(zk_ctx *ctx, const uint64_t *in, uint64_t n, uint64_t *out);
int32_t zk_ifft_host(zk_ctx *ctx, const uint64_t *in, uint64_t n, uint64_t *out);
/* fft_internal(values, omega) :21-46 with a caller-chosen omega: n not a power of two -> ZK_ERR_FFT_NOT_POW2 */
int32_t zk_fft_internal_host(zk_ctx *ctx, const uint64_t *in, uint64_t n, const uint64_t omega[4], uint64_t *out);

/* ---- UnivariatePolynomial  (polynomial/src/univariate_poly.rs) ------------------------------------------------
 * Coefficients lowest degree first, as `coefficients: Vec<F>` (:7-12).  Symbols only; the ABI version is unchanged.
 * Every result is exact field arithmetic, bit-identical to the reference. */
int32_t zk_upoly_upload(zk_ctx *ctx, const uint64_t *coeffs, uint64_t len, zk_upoly **out);    /* ::new :16-19 */
int32_t zk_upoly_len(const zk_upoly *p, uint64_t *out_len);
int32_t zk_upoly_download(zk_ctx *ctx, const zk_upoly *p, uint64_t *out_coeffs);               /* ::coefficients :21-23 */
int32_t zk_upoly_free(zk_ctx *ctx, zk_upoly *p);
/* Mul for &UnivariatePolynomial :186-209 -> new handle.  Either operand empty -> empty product (:190-192); otherwise
 * la + lb - 1 coefficients, trailing zeros kept ([0] * [1,2,3] = [0,0,0]).  a == b squares; the operands are not modified.
 * Asynchronous.  Small operands take a direct convolution, the others three fused NTTs of N = 2^ceil(log2(la+lb-1)) points.
 * DIVERGENCE: N > 2^two_adicity, N > 2^40 or N > 2^32 (the largest planned transform) -> ZK_ERR_UNSUPPORTED, where the
 * reference still computes the product by its quadratic loop. */
int32_t zk_upoly_mul(zk_ctx *ctx, const zk_upoly *a, const zk_upoly *b, zk_upoly **out);
/* ::evaluate :29-40 (Horner); the empty polynomial evaluates to 0.  One host wait. */
int32_t zk_upoly_evaluate(zk_ctx *ctx, const zk_upoly *p, const uint64_t x[4], uint64_t out[4]);
/* value-semantics form of Mul: out gets la + lb - 1 elements, nothing when la or lb is 0 (out may then be NULL).  The length
 * rule above is checked before the inputs are read. */
int32_t zk_upoly_mul_host(zk_ctx *ctx, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, uint64_t *out);
/* Add for &UnivariatePolynomial :157-184 -> new handle: an empty operand gives a copy of the other, otherwise max(la, lb) coefficients
 * added elementwise, nothing trimmed.  Asynchronous. */
int32_t zk_upoly_add(zk_ctx *ctx, const zk_upoly *a, const zk_upoly *b, zk_upoly **out);
/* ::interpolate :43-49 (xs = F::from(0 .. n-1)) -> new handle of exactly n coefficients, trailing zeros kept; n = 0: empty.  ys is a
 * device vector of n values.  Asynchronous.  O(n log^2 n): closed-form weights, then a subproduct tree.
 * DIVERGENCE: 2^ceil(log2 n) > 2^two_adicity or > 2^32 (the largest transform the tree needs) -> ZK_ERR_UNSUPPORTED, checked
 * before anything is read or allocated, where the reference still computes the result by its cubic loop. */
int32_t zk_upoly_interpolate(zk_ctx *ctx, const zk_upoly *ys, zk_upoly **out);
/* ::interpolate_xy :54-80 -> new handle: sum over i < m = min(nx, ny) of y_i L_i(x), each L_i over all nx points; nx coefficients,
 * or empty when m = 0.  A repeated x at some i < m (x_i = x_j, j != i) -> ZK_ERR_PANIC_INVERSE, where the reference panics on
 * (x_i - x_j).inverse().unwrap() (:68); repeats among indices >= m are no error (never inverted).  One host wait (that check); on
 * an error nothing is returned.  O(nx log^2 nx) for the tree; the weights' denominators prod_{j != i} (x_i - x_j) = M'(x_i) come
 * from the multipoint evaluation's tree path, O(nx log^2 nx), from ZK_UPOLY_INTERP_XY_TREE_MIN points on (where that path's length
 * rule allows it), and from an O(nx m) kernel below it: the same bits either way.  DIVERGENCE: the length rule of
 * zk_upoly_interpolate, with n = nx. */
int32_t zk_upoly_interpolate_xy(zk_ctx *ctx, const zk_upoly *xs, const zk_upoly *ys, zk_upoly **out);
/* value-semantics forms: out gets n (resp. nx, when nx and ny > 0) elements; nothing is written for an empty result (out may
 * then be NULL).  The length rule is checked before the inputs are read. */
int32_t zk_upoly_interpolate_host(zk_ctx *ctx, const uint64_t *ys, uint64_t n, uint64_t *out);
int32_t zk_upoly_interpolate_xy_host(zk_ctx *ctx, const uint64_t *xs, uint64_t nx, const uint64_t *ys, uint64_t ny, uint64_t *out);
/* Multipoint evaluation -> new handle of n = len(xs) values, out[i] = p.evaluate(xs[i]) (::evaluate :29-40); xs is a device vector
 * of n points (a zk_upoly doubles as a vector of field elements, as ys does for interpolate).  The empty polynomial gives n zeros,
 * n = 0 the empty handle; p == xs is allowed; the operands are not modified.  Asynchronous, no host wait.  Two paths with the same
 * bits: a direct one, O(n L) for L = len(p) (one lane per point, Horner over coefficient tiles in LDS, the coefficients split
 * over a second grid axis when the points are few), and the transposed subproduct tree, O(N log^2 N) for
 * N = 2^ceil(log2 max(n, L, 1)); a cost model picks, ZK_UPOLY_EVALMANY_DIRECT_MAX overrides it.  The tree
 * path keeps every level of the tree, (log2 N - 7) N 32 bytes (416 MiB at N = 2^20, 8.5 GiB at 2^24), and about 20 N 32 bytes
 * around them.  Length rule, checked before anything is read or allocated: the tree path's largest transform is 2N points, so it
 * is available when 2N <= 2^min(two_adicity, 32); where it is not, the direct path runs for n L <= 2^40 (about 12 s) and
 * n L > 2^40 -> ZK_ERR_UNSUPPORTED.  An allocation that fails returns ZK_ERR_ALLOC and leaves nothing behind. */
int32_t zk_upoly_evaluate_many(zk_ctx *ctx, const zk_upoly *p, const zk_upoly *xs, zk_upoly **out);
/* value-semantics form: out gets n elements; n = 0 writes nothing (out may then be NULL).  After the input pointers the length rule
 * is checked first, before out and before anything is read. */
int32_t zk_upoly_evaluate_many_host(zk_ctx *ctx, const uint64_t *coeffs, uint64_t len, const uint64_t *xs, uint64_t n, uint64_t *out);
/* Division with remainder -> new handles q and r with a = q b + r.  The reference has no division; the definition follows its
 * conventions (degree() = len - 1, :88-94; nothing is ever trimmed; the empty vector is the zero polynomial): lengths, not values,
 * fix every shape.  With la = len(a), lb = len(b): lb = 0 -> ZK_ERR_BAD_ARG (nothing is launched); la < lb -> q empty and r a copy
 * of a; otherwise q has k = la - lb + 1 coefficients and r has lb - 1 (empty for lb = 1), zeros at the top of a or anywhere in q / r
 * are kept, and the leading coefficient b[lb - 1] is inverted: a zero there -> ZK_ERR_PANIC_INVERSE (a device flag, read by the
 * call's one host wait; nothing is returned).  a == b is allowed; the operands are not modified; q or r (not both) may be NULL
 * to skip that result and the work for it.  Three paths with the same bytes (the result is unique): one workgroup of schoolbook
 * long division with the remainder in LDS for la <= ZK_UPOLY_DIVREM_DIRECT_MAX (default 1023, at most 2048); for lb = 2 above that a backward
 * scan of q[j-1] = (a[j] - b0 q[j]) / b1 in three launches over chunks of 4096 (a read twice, q written once;
 * ZK_UPOLY_DIVREM_LINEAR = 0 turns it off); otherwise Newton: q = rev((rev(a) mod z^k) (1 / rev(b) mod z^k) mod z^k) on the
 * univariate product, and r from the low lb - 1 coefficients of q b alone.  Length rule, checked before anything is read or
 * allocated: with K = 2^ceil(log2 k) the Newton path is available when 2K <= 2^min(two_adicity, 32) (its largest products are
 * 2K-point transforms) and the remainder's product of min(lb - 1, k) by lb - 1 coefficients passes zk_upoly_mul's rule; where it
 * is not available and no other path applies -> ZK_ERR_UNSUPPORTED.  An allocation that fails returns ZK_ERR_ALLOC and leaves
 * nothing behind.  DESIGN.md section 11. */
int32_t zk_upoly_divrem(zk_ctx *ctx, const zk_upoly *a, const zk_upoly *b, zk_upoly **out_q, zk_upoly **out_r);
/* Power-series inverse -> new handle of the k coefficients of 1 / f mod z^k (coefficients of f beyond len(f) count as zero), by
 * Newton steps on the univariate product.  k = 0 gives the empty handle; f empty -> ZK_ERR_PANIC_INVERSE (no wait); f[0] = 0 ->
 * ZK_ERR_PANIC_INVERSE (the device flag, one host wait).  Length rule: 2K <= 2^min(two_adicity, 32) for K = 2^ceil(log2 k), else
 * ZK_ERR_UNSUPPORTED. */
int32_t zk_upoly_inverse_series(zk_ctx *ctx, const zk_upoly *f, uint64_t k, zk_upoly **out);
/* value-semantics forms: out_q gets k (0 for la < lb) and out_r lb - 1 (la for la < lb) elements, out k elements; a pointer for an
 * empty result may be NULL.  After the input pointers the length rule is checked first, before the out pointers and before
 * anything is read. */
int32_t zk_upoly_divrem_host(zk_ctx *ctx, const uint64_t *a, uint64_t la, const uint64_t *b, uint64_t lb, uint64_t *out_q, uint64_t *out_r);
int32_t zk_upoly_inverse_series_host(zk_ctx *ctx, const uint64_t *f, uint64_t lf, uint64_t k, uint64_t *out);
/* Errors of the eighteen: null pointers -> ZK_ERR_BAD_ARG; a handle of another context -> ZK_ERR_CONTEXT_MISMATCH. */

/* ---- CoeffMultilinearPolynomial, dense  (polynomial/src/multilinear/coefficient_form.rs) -------------------------------
 * A zk_cmle made by upload or interpolate holds all 2^n_vars coefficients, index = key (key bit v <-> variable v, selector_to_index
 * :418-430), zeros included: the form interpolate produces, which has every key present (:200-216).  A partially evaluated one holds
 * the keys that are left (next section, with partial_evaluate, relabel, scalar_multiply, Add and Mul).  Elements in Montgomery form
 * like everywhere else.  ::new(terms), whose result lacks keys in no regular pattern, is not offered.  Symbols only; the ABI version
 * is unchanged. */
int32_t zk_cmle_upload(zk_ctx *ctx, uint64_t n_vars, const uint64_t *coeffs, uint64_t len, zk_cmle **out);  /* len != 2^n_vars -> ZK_ERR_EVAL_LEN */
int32_t zk_cmle_download(zk_ctx *ctx, const zk_cmle *p, uint64_t *out_coeffs);                              /* zk_cmle_len elements: 2^n_vars unless partially evaluated */
int32_t zk_cmle_n_vars(const zk_cmle *p, uint64_t *out);
int32_t zk_cmle_free(zk_ctx *ctx, zk_cmle *p);
/* ::interpolate :200-216 of the 2^n values of a table (MSB-first: table index bit n-1-v <-> variable v) -> new handle of n_vars =
 * max(n, 1): a table of one value is the reference's len == 1 case ({0: v, 1: -v}, bit_count_for_n_elem(1) = 1, :517-523).
 * Asynchronous; the table is left intact.  A Moebius transform in three crossings of the table at 2^24 (cmle_kernels.cuh). */
int32_t zk_cmle_interpolate(zk_ctx *ctx, const zk_mle *values, zk_cmle **out);
/* value-semantics form for any len: *out_n_vars = bit length of len - 1 (at least 1), values past len count as zero; out_coeffs
 * gets 2^*out_n_vars elements.  len == 0: *out_n_vars = 0 and nothing is written (the reference's empty map; out_coeffs may be
 * NULL).  len > 2^40 -> ZK_ERR_UNSUPPORTED before anything is read. */
int32_t zk_cmle_interpolate_host(zk_ctx *ctx, const uint64_t *values, uint64_t len, uint64_t *out_n_vars, uint64_t *out_coeffs);
/* ::to_evaluation_form :340-347 -> new table, as zk_coeff_to_evaluation computes it from the same terms.  n_vars == 0 ->
 * ZK_ERR_EVAL_LEN (as zk_coeff_to_evaluation).  Asynchronous. */
int32_t zk_cmle_to_evaluation(zk_ctx *ctx, const zk_cmle *p, zk_mle **out);
/* ::evaluate_slice :39-69: n_vars == 0 -> the coefficient of key 0; n_point < n_vars -> ZK_ERR_EVAL_ASSIGNMENT; assignments past
 * n_vars are ignored; assignment v goes to key bit v.  One host wait. */
int32_t zk_cmle_evaluate(zk_ctx *ctx, const zk_cmle *p, const uint64_t *point, uint64_t n_point, uint64_t out[4]);
/* ::to_bytes :131-139 -> 4 + 40 * 2^n_vars bytes: n_vars as u32 big-endian, then per key ascending the key as u64 big-endian and
 * the canonical coefficient as 32 bytes big-endian.  One host wait. */
int32_t zk_cmle_to_bytes(zk_ctx *ctx, const zk_cmle *p, uint8_t *out_bytes);
/* Errors of this section: null pointers -> ZK_ERR_BAD_ARG; a handle of another context -> ZK_ERR_CONTEXT_MISMATCH; n_vars > 40 ->
 * ZK_ERR_UNSUPPORTED.  On an error no handle is returned. */

/* ---- CoeffMultilinearPolynomial, dense: algebra  (coefficient_form.rs :72-123, :272-282, :350-415) -------------------------
 * Which keys a BTreeMap holds shows in the reference's results (to_bytes, ==, the n_vars Add picks), so the handle tracks it.  A
 * fresh handle has every key.  partial_evaluate of a set S of variables removes exactly the keys with a bit in S and leaves every
 * other key present (:93-99), so the present keys of a handle are always {k : k & fixed == 0} for a mask `fixed`.  The handle
 * stores their coefficients in ascending key order: zk_cmle_len = 2^(n_vars - popcount(fixed)) elements, element j being key
 * pdep(j, ~fixed) (the bits of j spread over the positions not in fixed, lowest first).  With fixed == 0 nothing differs from the
 * section above.  On a handle with fixed != 0:
 *   zk_cmle_download   writes zk_cmle_len elements, ascending key order;
 *   zk_cmle_to_bytes   writes 4 + 40 * zk_cmle_len bytes, the records' keys being pdep(j, ~fixed) (ascending, as the BTreeMap's);
 *   zk_cmle_evaluate   checks n_point >= n_vars against the full n_vars and ignores the coordinates of the fixed variables;
 *   zk_cmle_to_evaluation and zk_bench_cmle return ZK_ERR_UNSUPPORTED until the handle is relabelled.
 * DIVERGENCE (Mul only): the reference skips every pair with a zero coefficient (:393-395), so the keys that only such pairs reach
 * are ABSENT from its product; zk_cmle_mul holds them with coefficient zero.  The two are equal as polynomials, and key for key and
 * byte for byte equal when no operand coefficient is zero.  The other four operations reproduce the reference's key set exactly. */
int32_t zk_cmle_fixed_mask(const zk_cmle *p, uint64_t *out);   /* bit v set <-> variable v has been fixed: no present key has bit v */
int32_t zk_cmle_len(const zk_cmle *p, uint64_t *out);          /* number of present keys */
/* ::partial_evaluate :72-104 -> new handle, p unchanged.  Assignment i is (selector i, values[4i..4i+4)); the selectors are bool bytes
 * (nonzero = true), concatenated, selector i being selector_lens[i] long.  In the caller's order, per assignment: selector longer than
 * n_vars -> skipped (:87-89); any other length != n_vars -> ZK_ERR_SELECTOR_LEN; not exactly one byte set -> ZK_ERR_SELECTOR_SINGLE
 * (get_variable_indexes :285-304); a variable already fixed in p or assigned earlier in this call -> nothing happens, so the first
 * assignment of a variable wins.  The result has p's n_vars and fixed | {assigned variables}; n_assign == 0 -> an equal copy.
 * Asynchronous; ceil(s / 3) launches for s newly fixed variables, reading the source once (cmle_kernels.cuh). */
int32_t zk_cmle_partial_evaluate(zk_ctx *ctx, const zk_cmle *p, const uint8_t *selectors, const uint64_t *selector_lens,
                                 const uint64_t *values, uint64_t n_assign, zk_cmle **out);
/* ::relabel :109-123, IN PLACE (the reference consumes self): the variables still present move down in order, n_vars becomes
 * n_vars - popcount(fixed) and fixed 0.  No device work: the stored vector is already the relabelled one.  n_vars == 0, and any
 * handle with fixed == 0 (every variable present in some key), is left as it is. */
int32_t zk_cmle_relabel(zk_ctx *ctx, zk_cmle *p);
/* ::scalar_multiply :272-282 -> new handle with p's n_vars and fixed mask: every present coefficient times s.  Asynchronous. */
int32_t zk_cmle_scalar_multiply(zk_ctx *ctx, const zk_cmle *p, const uint64_t s[4], zk_cmle **out);
/* Add for & :350-373 -> new handle: the operand with more keys copied (b on a tie: its n_vars is the result's, :360-365) and the
 * other summed into its low keys.  Both operands need fixed == 0, else ZK_ERR_UNSUPPORTED (the union of two masked key sets is not
 * of the form above; relabel first).  Asynchronous. */
int32_t zk_cmle_add(zk_ctx *ctx, const zk_cmle *a, const zk_cmle *b, zk_cmle **out);
/* Mul for & :375-415 -> new handle of n_a + n_b variables, a's variables first: out[i | j << n_a] = a[i] * b[j]; n_a == 0 or n_b == 0
 * is the scalar path (:380-384).  Zero coefficients: see DIVERGENCE above.  Both operands need fixed == 0, else ZK_ERR_UNSUPPORTED;
 * n_a + n_b > 40 -> ZK_ERR_UNSUPPORTED before anything is allocated.  Asynchronous. */
int32_t zk_cmle_mul(zk_ctx *ctx, const zk_cmle *a, const zk_cmle *b, zk_cmle **out);
/* Errors of this section: null pointers -> ZK_ERR_BAD_ARG; a handle of another context -> ZK_ERR_CONTEXT_MISMATCH.  On an error no
 * handle is returned and p is unchanged. */

/* ---- batch inversion and running products over tables (no reference item; definition: tests/batch_inverse_ref.py) ------------
 * Montgomery's trick on the device (zk_amd/csrc/inv_kernels.cuh): one field inversion per call, about 4
 * multiplications and 96 bytes per element, three launches -- one for tables of at most one chunk (2048 elements; the switch
 * ZK_BATCH_INV_ONE_LAUNCH_MAX).  A field inverse is unique, so every path gives the bits of x^(p-2).  A zero denominator is no error:
 * it is written as zero and counted, at the cost of any other value. */
/* no reference item; definition: tests/batch_inverse_ref.py batch_inverse.
   out[i] = (t[i] + shift)^-1, and 0 where t[i] + shift == 0 (ark-ff batch_inversion's rule: zeros are skipped, not an error).
   shift NULL = 0.  out may be t itself (in place) or another table of the same n_vars.
   out_zeros NULL: stream-ordered, no host wait.  Non-NULL: receives the number of zero denominators; the call waits for the stream. */
int32_t zk_mle_batch_inverse(zk_ctx *ctx, const zk_mle *t, const uint64_t *shift, zk_mle *out, uint64_t *out_zeros);
/* no reference item; definition: tests/batch_inverse_ref.py batch_inverse.
   the same on a vector of any length (0 included: an empty handle); *out is a new handle */
int32_t zk_upoly_batch_inverse(zk_ctx *ctx, const zk_upoly *v, const uint64_t *shift, zk_upoly **out, uint64_t *out_zeros);
/* no reference item; definition: tests/batch_inverse_ref.py prefix_product.
   exclusive (inclusive == 0): out[0] = 1, out[i] = t[0]...t[i-1];  inclusive: out[i] = t[0]...t[i].  Plain products: a zero
   propagates.  out may be t.  out_total NULL: no host wait; non-NULL: the product of all 2^n_vars elements, waits for the stream. */
int32_t zk_mle_prefix_product(zk_ctx *ctx, const zk_mle *t, int32_t inclusive, zk_mle *out, uint64_t *out_total);
/* no reference item; definition: tests/batch_inverse_ref.py batch_inverse.
   value-semantics form (upload, compute, download), n >= 0 (n == 0: in and out may be NULL); out may be in; out_zeros may be NULL;
   n > 2^40 -> ZK_ERR_UNSUPPORTED */
int32_t zk_batch_inverse_host(zk_ctx *ctx, const uint64_t *in, uint64_t n, const uint64_t *shift, uint64_t *out, uint64_t *out_zeros);
/* Errors of this section, in this order: a NULL ctx, t, v or out -> ZK_ERR_BAD_ARG; a handle of another context ->
 * ZK_ERR_CONTEXT_MISMATCH; out->n_vars != t->n_vars -> ZK_ERR_BAD_ARG.  On an error nothing is launched and no handle is returned. */

/* ---- binary Merkle commitments over tables with batched openings (no reference item; definition: tests/merkle_ref.py) ----------
 * leaf[i] = Keccak256(be32(c_0[i]) || ... || be32(c_{k-1}[i])) over k columns of 2^n elements (be32: the 32-byte big-endian canonical
 * integer, the per-element image of to_bytes; the hash is zk_keccak256's), level[d+1][j] = Keccak256(level[d][2j] || level[d][2j+1]),
 * root = level[n][0] (n = 0: the one leaf).  No domain-separation bytes: n and k are part of the statement and the verifier takes both,
 * so a node is never read as a leaf.  Every level stays on the device (zk_amd/csrc/merkle_kernels.cuh); the
 * opening of row i is the row and the n siblings level[d][(i >> d) ^ 1], bottom up.  The switch ZK_MERKLE_FUSE_LEVELS selects between
 * one launch per level and fused sub-tree stages; both give the same bytes.  The statement digest of the GKR driver (4-ary, 128-byte
 * leaves) is another format and is unchanged. */
typedef struct zk_merkle zk_merkle;   /* device-resident digests of every level of one commitment */
/* no reference item; definition: tests/merkle_ref.py commit.
   stream-ordered, no host wait; the handle does not keep the columns alive or refer to them afterwards */
int32_t zk_merkle_commit(zk_ctx *ctx, const zk_mle *const *columns, uint32_t n_columns, zk_merkle **out);
int32_t zk_merkle_free(zk_merkle *m);                       /* as zk_upoly_free: back to its context's pool, NULL is fine */
int32_t zk_merkle_n_vars(const zk_merkle *m, uint32_t *out);
int32_t zk_merkle_n_columns(const zk_merkle *m, uint32_t *out);
int32_t zk_merkle_root(zk_ctx *ctx, const zk_merkle *m, uint8_t out[32]);                 /* waits for the stream */
/* all 2^(n-level) digests of one level, 32 bytes each, to the host (tests, and users who ship the top of the tree) */
int32_t zk_merkle_level(zk_ctx *ctx, const zk_merkle *m, uint32_t level, uint8_t *out);
/* no reference item; definition: tests/merkle_ref.py open.
   n_queries host indices (from the transcript) -> paths (n_queries * n * 32 bytes) and, when columns != NULL, the opened rows
   (n_queries * n_columns elements, Montgomery limbs like every element that crosses this ABI).  One gather launch for all
   queries, one download; duplicates allowed; n_queries == 0 is a no-op.  The columns are the caller's claim: not re-hashed. */
int32_t zk_merkle_open(zk_ctx *ctx, const zk_merkle *m, const zk_mle *const *columns, uint32_t n_columns,
                       const uint64_t *indices, uint64_t n_queries, uint64_t *out_rows, uint8_t *out_paths);
/* no reference item; definition: tests/merkle_ref.py verify.
   host only, needs no context and no GPU: *out_ok = 1 / 0 */
int32_t zk_merkle_verify_host(int32_t field, const uint8_t root[32], uint32_t n_vars, uint32_t n_columns, uint64_t index,
                              const uint64_t *row, const uint8_t *path, int32_t *out_ok);
/* Errors of this section, in this order: NULL pointers and n_columns == 0 -> ZK_ERR_BAD_ARG; a handle of another context ->
 * ZK_ERR_CONTEXT_MISMATCH; columns of differing n_vars (in open: differing from the commitment's) -> ZK_ERR_ARITY_MISMATCH;
 * n_columns > 1024 -> ZK_ERR_UNSUPPORTED; level > n, an index >= 2^n, an n_columns in open that differs from the commitment's ->
 * ZK_ERR_BAD_ARG; a row element in verify_host that is not fully reduced -> ZK_ERR_BAD_ARG (as zk_fe_from_canonical refuses it; an
 * unknown field -> ZK_ERR_BAD_FIELD before everything else).  On an error nothing is launched and no handle is returned. */

/* ---- FRI low-degree proofs: coset LDE, fold by 2^a, prover, host verifier (no reference item; definition: tests/fri_ref.py) --------
 * Parameters: log_degree d (the polynomial has at most 2^d coefficients), log_blowup b (1..8), log_arity a (1..3), log_final f (f < d,
 * a divides d - f), n_queries Q (1..1024), a non-zero shift, a 32-byte seed; R = (d - f) / a rounds.  Layer r is 2^(d+b-a r) evaluations
 * in natural order over the coset shift^(2^(a r)) * <root_of_unity(2^(d+b-a r))>; a fold maps
 *   out[i] = (v[i] + v[i+N/2]) / 2 + beta (v[i] - v[i+N/2]) / (2 s w^i)
 * a times with (s, beta), (s^2, beta^2), (s^4, beta^4).  Layer r is committed as a Merkle tree (the section above) over its 2^a column
 * views v[j M : (j+1) M], M = N / 2^a, so that row i holds the 2^a inputs of output i.  The transcript (zk_transcript's sponge) absorbs the
 * seed, the field id, d, b, a, f, Q as 8-byte big-endian integers and be32(shift); per round the root, then draws beta; then the 2^f final
 * coefficients as be32; every query index is bytes 24..32 of a challenge, big endian, masked to M_0 - 1.  Proof bytes: R roots, 2^f final
 * coefficients as be32, then per query and per round the row (2^a x be32) and the path (log2 M_r x 32 bytes).  DESIGN.md section 14. */
/* no reference item; definition: tests/fri_ref.py lde.
   the evaluations of p (at most 2^log_n coefficients) over shift * <root_of_unity(2^log_n)>, natural order, as a new table of log_n variables */
int32_t zk_fri_lde(zk_ctx *ctx, const zk_upoly *p, uint32_t log_n, const uint64_t shift[4], zk_mle **out);
/* no reference item; definition: tests/fri_ref.py fold.
   `in` over the coset of `shift` -> `out` (n_vars - log_arity variables, another table) at the challenge beta; stream-ordered, `in` is left
   intact.  One fused launch, or log_arity binary launches under ZK_FRI_FUSED_FOLD = 0: the same bytes */
int32_t zk_fri_fold(zk_ctx *ctx, const zk_mle *in, uint32_t log_arity, const uint64_t shift[4], const uint64_t beta[4], zk_mle *out);
/* no reference item; definition: tests/fri_ref.py proof_bytes.
   32 (R + 2^f + Q sum_r (2^a + log2 M_r)); host only */
int32_t zk_fri_proof_bytes(uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final, uint32_t n_queries, uint64_t *out);
/* no reference item; definition: tests/fri_ref.py prove.
   the whole proof into out_proof (zk_fri_proof_bytes bytes): LDE, per round commit / one host wait for the root / fold, the final
   coefficients, one gather launch per layer for all queries.  p is left intact */
int32_t zk_fri_prove(zk_ctx *ctx, const zk_upoly *p, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final,
                     uint32_t n_queries, const uint64_t shift[4], const uint8_t seed[32], uint8_t *out_proof);
/* no reference item; definition: tests/fri_ref.py verify.
   host only, needs no context and no GPU: *out_ok = 1 / 0.  A proof element that is not canonical (>= p) makes *out_ok = 0, not an error */
int32_t zk_fri_verify_host(int32_t field, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final,
                           uint32_t n_queries, const uint64_t shift[4], const uint8_t seed[32], const uint8_t *proof, uint64_t proof_len,
                           int32_t *out_ok);
/* Errors of this section, in this order: a NULL pointer -> ZK_ERR_BAD_ARG; an unknown field -> ZK_ERR_BAD_FIELD; a handle of another
 * context -> ZK_ERR_CONTEXT_MISMATCH; log_arity outside 1..3, log_blowup outside 1..8, n_queries outside 1..1024, log_final >= log_degree,
 * log_arity not dividing log_degree - log_final, log_degree > 40, more than 2^log_degree (zk_fri_lde: 2^log_n) coefficients, a shift
 * (or beta) that is zero (beta may be) or not fully reduced, an `out` of the wrong size or out == in, proof_len != zk_fri_proof_bytes ->
 * ZK_ERR_BAD_ARG; a domain larger than 2^two_adicity -> ZK_ERR_FFT_NO_ROOT; zk_fri_fold with n_vars < log_arity -> ZK_ERR_EVAL_LEN; a
 * failed allocation -> ZK_ERR_ALLOC with nothing left behind.  On an error nothing is returned. */

/* ---- FRI polynomial commitment: DEEP quotient, commit, open at a point, host verifier (no reference item; definition: tests/pcs_ref.py) ----
 * Parameters: k >= 1 polynomials of at most 2^d coefficients, d, b, a, f, Q with FRI's meaning and limits (the section above), k 2^a <= 1024
 * (the Merkle leaf's column limit), a non-zero shift s, a 32-byte seed; N = 2^(d+b), M = N / 2^a, w = root_of_unity(N), x_i = s w^i.
 * commit: F_c = zk_fri_lde(f_c, d + b, s); one Merkle tree of M rows over the k 2^a column views, column c 2^a + j = F_c[j M : (j+1) M] (FRI's
 * own row layout: row i holds every value the verifier needs at FRI query index i); the commitment is the root.  open at z (off the domain:
 * z^N != s^N): y_c = f_c(z); the transcript absorbs the seed, the field id, k, d, b, a, f, Q as 8-byte big-endian integers, be32(s), the
 * root, be32(z), be32(y_0) .. be32(y_{k-1}), then draws alpha (a field element) and fri_seed (a challenge);
 *   q[i] = (sum_c alpha^c (F_c[i] - y_c)) / (x_i - z)
 * has fewer than 2^d coefficients exactly when every y_c is right.  FRI's bound is 2^d coefficients, one more, so the layer that
 * zk_fri_prove's prover proves low-degree under fri_seed is x_i q[i], the evaluations of X q(X): it has at most 2^d coefficients exactly
 * when q has at most 2^d - 1 (q alone would let an f_c of 2^d + 1 coefficients through).  Proof bytes: that FRI proof, then per query t
 * the row idx_t of the commitment tree (k 2^a x be32) and its path ((d + b - a) x 32 bytes).  The values are the public claim, beside
 * the proof.  The verifier checks the FRI part, every tree opening and, for every j < 2^a, that entry j of the FRI part's round-0 row
 * equals x q formed from the opened row at x = x_{idx_t + j M}.  DESIGN.md section 15. */
typedef struct zk_pcs zk_pcs;   /* one commitment: the k LDE tables, their tree and a copy of the coefficients, on the device */
/* no reference item; definition: tests/pcs_ref.py quotient.
   out[i] = (sum_c alpha^c (columns[c][i] - values[c])) / (shift w^i - z) over the 2^n_vars points of the coset; values: n_columns x 4 limbs.
   Public in its own right, for callers who build other protocols.  Stream-ordered, no host wait; `out` is another table than every
   column; the columns are left intact.  One launch up to 2^11 points, three above (zk_amd/csrc/pcs_kernels.cuh) */
int32_t zk_deep_quotient(zk_ctx *ctx, const zk_mle *const *columns, uint32_t n_columns, const uint64_t shift[4], const uint64_t z[4],
                         const uint64_t *values, const uint64_t alpha[4], zk_mle *out);
/* no reference item; definition: tests/pcs_ref.py commit.
   stream-ordered, no host wait; the handle owns what it needs and does not refer to the polynomials afterwards */
int32_t zk_pcs_commit(zk_ctx *ctx, const zk_upoly *const *polys, uint32_t k, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity,
                      const uint64_t shift[4], zk_pcs **out);
int32_t zk_pcs_free(zk_pcs *h);                              /* as zk_merkle_free: back to its context's pool, NULL is fine */
int32_t zk_pcs_n_polys(const zk_pcs *h, uint32_t *out);
int32_t zk_pcs_root(zk_ctx *ctx, const zk_pcs *h, uint8_t out[32]);                      /* waits for the stream */
/* no reference item; definition: tests/pcs_ref.py proof_bytes.
   zk_fri_proof_bytes(d, b, a, f, Q) + 32 Q (k 2^a + d + b - a); host only */
int32_t zk_pcs_proof_bytes(uint32_t k, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final, uint32_t n_queries,
                           uint64_t *out);
/* no reference item; definition: tests/pcs_ref.py prove.
   the k values f_c(z) into out_values (k x 4 Montgomery limbs) and the proof into out_proof (zk_pcs_proof_bytes bytes): the values (one
   download, one host wait), the quotient, zk_fri_prove's rounds on it, and the commitment's rows and paths gathered by one launch joined
   to the prover's final download.  The handle is left intact: it can be opened again at another point */
int32_t zk_pcs_open(zk_ctx *ctx, const zk_pcs *h, const uint64_t z[4], uint32_t log_final, uint32_t n_queries, const uint8_t seed[32],
                    uint64_t *out_values, uint8_t *out_proof);
/* no reference item; definition: tests/pcs_ref.py verify.
   host only, needs no context and no GPU: *out_ok = 1 / 0.  A proof element that is not canonical (>= p) makes *out_ok = 0, not an error */
int32_t zk_pcs_verify_host(int32_t field, uint32_t k, uint32_t log_degree, uint32_t log_blowup, uint32_t log_arity, uint32_t log_final,
                           uint32_t n_queries, const uint64_t shift[4], const uint8_t seed[32], const uint8_t root[32], const uint64_t z[4],
                           const uint64_t *values, const uint8_t *proof, uint64_t proof_len, int32_t *out_ok);
/* Errors of this section, in this order: a NULL pointer, k or n_columns == 0 -> ZK_ERR_BAD_ARG; an unknown field -> ZK_ERR_BAD_FIELD; a
 * handle of another context -> ZK_ERR_CONTEXT_MISMATCH; log_arity outside 1..3, log_blowup outside 1..8, n_queries outside 1..1024,
 * log_arity > log_degree, log_final >= log_degree, log_arity not dividing log_degree - log_final, log_degree > 40, k 2^a > 1024 (zk_deep_quotient:
 * n_columns > 1024), more than 2^log_degree coefficients, columns and `out` of differing n_vars or `out` one of the columns, a shift that
 * is zero, a shift, z, alpha or value that is not fully reduced, a z on the domain (z^N == shift^N), proof_len != zk_pcs_proof_bytes ->
 * ZK_ERR_BAD_ARG; a domain larger than 2^two_adicity -> ZK_ERR_FFT_NO_ROOT; a failed allocation -> ZK_ERR_ALLOC with nothing left behind.
 * On an error nothing is returned. */

/* ---- multilinear polynomial commitment: BaseFold over the FRI layers (no reference item; definition: tests/mlpcs_ref.py) ----------------
 * Parameters: a table t of 2^n values (n >= 1; variable 0 = the index's top bit), b = log2 of the blowup (1..8), f = log2 of the final
 * polynomial's length (0 <= f < n), Q queries (1..1024), a non-zero shift s, a 32-byte seed; R = n - f rounds, every fold is by 2; n + b
 * at most the field's two-adicity.  No security level is claimed for any choice: as with zk_fri_*, b and Q are the caller's business.
 * Commit: c = the coefficient form of t (zk_cmle_interpolate: key bit v <-> variable v), F_0 = its coset LDE over 2^(n+b) points, one
 * Merkle tree over the two column views F_0[0:M_0], F_0[M_0:2 M_0] (layer 0 of zk_fri_prove at arity 2); the commitment is its root.
 * Open at z = (z_0 .. z_{n-1}), any elements: v = t(z); transcript: seed; be64 of field id, n, b, f, Q; be32(s); root_0; be32(z_j);
 * be32(v).  Round r: (r >= 1: root_r of F_r, absorbed;) h_r(X) = sum_x' T_r(X, x') eq((X, x'), (z_r ..)) c_r for X = 0, 1, 2, absorbed;
 * beta_r = sample_field_element; T_{r+1} = partial_evaluate(0, [beta_r]) of T_r and F_{r+1} = the FRI fold of F_r at beta_r -- the same
 * variable, so F_r stays the LDE of the coefficient form of T_r.  Then the first 2^f coefficients of F_R (the coefficient form of T_R),
 * absorbed, and Q query indices as FRI draws them.  Proof: h_0 | r = 1..R-1: root_r, h_r | final | per query, per round: the row
 * (2 x be32) and the path (n + b - 1 - r digests), layer 0 from the commitment's own tree; 32 (3R + R - 1 + 2^f) + 32 Q sum_r (2 + n + b
 * - 1 - r) bytes.  v is the public claim, beside the proof.  The verifier checks the length, canonical elements, h_r(0) + h_r(1) =
 * claim_r and claim_{r+1} = h_r(beta_r), claim_R = prod_j eq1(beta_j, z_j) times the final polynomial at (z_R ..), and every query as
 * zk_fri_verify_host does with the sumcheck's betas.  DESIGN.md section 16. */
typedef struct zk_mlpcs zk_mlpcs;   /* one commitment: a copy of the table, F_0 and its tree, on the device */
/* no reference item; definition: tests/mlpcs_ref.py commit.
   stream-ordered, no host wait; the handle owns copies and does not refer to the table afterwards */
int32_t zk_mlpcs_commit(zk_ctx *ctx, const zk_mle *table, uint32_t log_blowup, const uint64_t shift[4], zk_mlpcs **out);
int32_t zk_mlpcs_free(zk_mlpcs *h);                          /* as zk_pcs_free: back to its context's pool, NULL is fine */
int32_t zk_mlpcs_n_vars(const zk_mlpcs *h, uint32_t *out);
int32_t zk_mlpcs_root(zk_ctx *ctx, const zk_mlpcs *h, uint8_t out[32]);                  /* waits for the stream */
/* no reference item; definition: tests/mlpcs_ref.py proof_bytes.  host only */
int32_t zk_mlpcs_proof_bytes(uint32_t n_vars, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries, uint64_t *out);
/* no reference item; definition: tests/mlpcs_ref.py prove.
   v = t(point) into out_value (Montgomery limbs) and the proof into out_proof (zk_mlpcs_proof_bytes bytes).  One host wait per round:
   behind the codeword's fold, the layer's tree and the round's sumcheck launch one download brings the root and the round's sums.  The
   handle is left intact: it can be opened again at other points, with another log_final and n_queries.  The sumcheck launch is the
   round kernel of zk_amd/csrc/mlpcs_kernels.cuh (no eq table; the fold of T_{r-1} joined to the sums of T_r) or, with ZK_MLPCS_ROUND=0,
   zk_eq_table and per round the launches of zk_round_sums and zk_mle_fold_into: the same bytes */
int32_t zk_mlpcs_open(zk_ctx *ctx, const zk_mlpcs *h, const uint64_t *point, uint64_t n_point, uint32_t log_final, uint32_t n_queries,
                      const uint8_t seed[32], uint64_t out_value[4], uint8_t *out_proof);
/* no reference item; definition: tests/mlpcs_ref.py verify.
   host only, needs no context and no GPU: *out_ok = 1 / 0; proof_len is checked against zk_mlpcs_proof_bytes before anything is read.
   A proof element that is not canonical (>= p) makes *out_ok = 0, not an error */
int32_t zk_mlpcs_verify_host(int32_t field, uint32_t n_vars, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries,
                             const uint64_t shift[4], const uint8_t seed[32], const uint8_t root[32], const uint64_t *point,
                             const uint64_t value[4], const uint8_t *proof, uint64_t proof_len, int32_t *out_ok);
/* no reference item; definition: tests/mlpcs_ref.py eq_sums.
   S_X = sum_{x'} t[X 2^(n-1) + x'] eq(x', tail), X = 0, 1, into out (2 x 4 Montgomery limbs); tail: n_vars - 1 elements (variables 1 ..;
   may be NULL for n_vars = 1).  What the opening's round kernel leaves of a round; public in its own right.  Waits for the stream; t is
   left intact */
int32_t zk_mle_eq_sums(zk_ctx *ctx, const zk_mle *t, const uint64_t *tail, uint64_t out[8]);
/* Errors of this section, in this order: a NULL pointer -> ZK_ERR_BAD_ARG; an unknown field -> ZK_ERR_BAD_FIELD; a handle of another
 * context -> ZK_ERR_CONTEXT_MISMATCH; n_point != n_vars -> ZK_ERR_EVAL_ARITY; log_blowup outside 1..8, n_queries outside 1..1024,
 * log_final >= n_vars, n_vars == 0 or > 40, a shift that is zero, a shift, point element, tail element or value that is not fully
 * reduced, proof_len != zk_mlpcs_proof_bytes -> ZK_ERR_BAD_ARG; n_vars + log_blowup above the two-adicity -> ZK_ERR_FFT_NO_ROOT (above
 * 40: ZK_ERR_UNSUPPORTED); a failed allocation -> ZK_ERR_ALLOC with nothing left behind.  On an error nothing is written. */

/* ---- batch multilinear commitment: k tables under one tree, m points, one opening (zk_amd/csrc/mlbatch.hip) ------
 * The reference has nothing like it; tests/mlbatch_ref.py defines every byte.  k tables t_c of 2^n values each (1 <= k <= 256; the same
 * n for all: tables of another size go into another commitment) are committed under ONE Merkle tree over the 2k column views of their
 * layers F_0^c (column 2c = F_0^c[0:M_0], 2c + 1 = F_0^c[M_0:2 M_0]; k = 1: zk_mlpcs_commit's root).  An opening at m points z_j
 * (1 <= m <= 16, repeats allowed) publishes the m x k matrix v[j][c] = t_c(z_j), absorbs seed | be64 of field id, n, b, f, Q, k, m |
 * be32(s) | root | every z_j | every v[j][c] (both j-major), draws lambda and gamma, and runs ONE BaseFold opening (the section above) of
 * T_0 = sum_c lambda^c t_c against E_0 = sum_j gamma^j eq(., z_j) with claim_0 = sum_j gamma^j sum_c lambda^c v[j][c]; the layer
 * F_0 = sum_c lambda^c F_0^c is never committed: a query opens the commitment's row of 2k elements and combines it with the same
 * powers of lambda.  Proof: as zk_mlpcs_open's with rows of 2k elements in round 0; 32 (3R + R - 1 + 2^f) + 32 Q ((2k + n + b - 1) +
 * sum_{r=1..R-1} (2 + n + b - 1 - r)) bytes.  The values are public, beside the proof. */
typedef struct zk_mlbatch zk_mlbatch;   /* one commitment: copies of the k tables, their layers F_0^c in one block and the tree, on the device */
/* no reference item; definition: tests/mlbatch_ref.py commit.
   stream-ordered, no host wait; the handle owns copies and does not refer to the tables afterwards */
int32_t zk_mlbatch_commit(zk_ctx *ctx, const zk_mle *const *tables, uint32_t k, uint32_t log_blowup, const uint64_t shift[4], zk_mlbatch **out);
int32_t zk_mlbatch_free(zk_mlbatch *h);                        /* as zk_mlpcs_free: NULL is fine */
int32_t zk_mlbatch_n_vars(const zk_mlbatch *h, uint32_t *out);
int32_t zk_mlbatch_n_tables(const zk_mlbatch *h, uint32_t *out);
int32_t zk_mlbatch_root(zk_ctx *ctx, const zk_mlbatch *h, uint8_t out[32]);                /* waits for the stream */
/* no reference item; definition: tests/mlbatch_ref.py proof_bytes.  host only */
int32_t zk_mlbatch_proof_bytes(uint32_t n_vars, uint32_t k, uint32_t n_points, uint32_t log_blowup, uint32_t log_final, uint32_t n_queries,
                               uint64_t *out);
/* no reference item; definition: tests/mlbatch_ref.py prove.
   points: n_points x n_vars elements; out_values: n_points x k elements (Montgomery limbs), v[j][c] = t_c(z_j); out_proof:
   zk_mlbatch_proof_bytes bytes.  Host waits: one for the root and the values, one per round from round 1 on (round 0's sums follow from
   the values' own), one for the final polynomial, one for the gathered rows.  The first fold of the codewords is
   k_ml_combine_fold (zk_amd/csrc/mlbatch_kernels.cuh: the combined layer 0 is never written) or, with ZK_MLBATCH_FUSE_FOLD=0, a
   zk_mle_lincomb into a scratch layer and FRI's fold: the same bytes.  The handle is left intact */
int32_t zk_mlbatch_open(zk_ctx *ctx, const zk_mlbatch *h, const uint64_t *points, uint32_t n_points, uint32_t log_final, uint32_t n_queries,
                        const uint8_t seed[32], uint64_t *out_values, uint8_t *out_proof);
/* no reference item; definition: tests/mlbatch_ref.py verify.
   host only, needs no context and no GPU: *out_ok = 1 / 0; proof_len is checked against zk_mlbatch_proof_bytes before anything is read.
   A proof element that is not canonical (>= p) makes *out_ok = 0, not an error */
int32_t zk_mlbatch_verify_host(int32_t field, uint32_t n_vars, uint32_t k, uint32_t n_points, uint32_t log_blowup, uint32_t log_final,
                               uint32_t n_queries, const uint64_t shift[4], const uint8_t seed[32], const uint8_t root[32],
                               const uint64_t *points, const uint64_t *values, const uint8_t *proof, uint64_t proof_len, int32_t *out_ok);
/* no reference item; definition: tests/mlbatch_ref.py lincomb.
   out[i] = sum_c coeffs[c] tables[c][i]: k tables of out's n_vars (0 .. 40), coeffs: k elements.  out may not alias a source
   (ZK_ERR_BAD_ARG).  Waits for the stream (the coefficients' staging); the sources are left intact */
int32_t zk_mle_lincomb(zk_ctx *ctx, const zk_mle *const *tables, uint32_t k, const uint64_t *coeffs, zk_mle *out);
/* no reference item; definition: tests/mlbatch_ref.py eq_sums_many.
   zk_mle_eq_sums at n_points tails in passes over t of up to kMlPointsPerPass points each: tails: n_points x (n_vars - 1) elements (may
   be NULL for n_vars = 1), out: n_points x 2 elements (S_0^j, S_1^j).  Waits for the stream; t is left intact */
int32_t zk_mle_eq_sums_many(zk_ctx *ctx, const zk_mle *t, const uint64_t *tails, uint32_t n_points, uint64_t *out);
/* Errors of this section, in zk_mlpcs_*'s order: a NULL pointer -> ZK_ERR_BAD_ARG; an unknown field -> ZK_ERR_BAD_FIELD; a handle or
 * table of another context -> ZK_ERR_CONTEXT_MISMATCH; the shapes as in the section above, k outside 1..256, n_points outside 1..16,
 * tables of different n_vars, a point element, coefficient, tail element or value that is not fully reduced -> ZK_ERR_BAD_ARG; then
 * ZK_ERR_FFT_NO_ROOT / ZK_ERR_UNSUPPORTED / ZK_ERR_ALLOC as above.  On an error nothing is written. */

/* ---- grand-product argument: a fused product tree and one sumcheck per layer (zk_amd/csrc/gprod.hip) -----------
 * The reference has nothing like it; tests/gprod_ref.py defines every byte.  P = prod_i (t[i] + shift) is shown to a verifier who is left
 * with ONE claim t(point) = claim, which the caller checks however it can (zk_mle_evaluate, or a zk_mlpcs_open at that point): what a
 * permutation, multiset-equality or memory-checking argument is built on.  Tree: V_n = t + shift, V_j[i] = V_{j+1}[i] V_{j+1}[i + 2^j]
 * (variable 0 = the index's top bit), P = V_0[0].  Layer j = 0 .. n - 1 turns the claim V_j(r_j) = c_j into one on V_{j+1} by a sumcheck
 * of eq(x, r_j) V_{j+1}(0, x) V_{j+1}(1, x) (degree 3, j rounds) and the two values a, b at its point; proof = per layer the 4 j round
 * evaluations, then a, b: 2 n^2 elements as 32-byte big-endian canonical integers.
 * BINDING: the argument does NOT absorb the table (prove_partial does not either): the 32-byte seed must bind it, e.g. the root of the
 * table's commitment; a shift drawn as a challenge must be drawn after that. */
/* no reference item; definition: tests/gprod_ref.py product_tree.
   *out = a new table of n_vars variables in heap order: out[0] = 1, out[2^j + i] = V_j[i] for 0 <= j < n_vars (so out[1] = P); shift NULL
   = 0.  Stream-ordered, no host wait; t is left intact */
int32_t zk_mle_product_tree(zk_ctx *ctx, const zk_mle *t, const uint64_t *shift, zk_mle **out);
/* 64 n_vars^2 */
int32_t zk_gprod_proof_bytes(uint32_t n_vars, uint64_t *out);
/* no reference item; definition: tests/gprod_ref.py prove.
   out_product = P, out_proof = zk_gprod_proof_bytes(n_vars) bytes; out_point (n_vars elements) and out_claim are what the verifier will
   derive, so a caller can start its opening without running the verifier.  shift NULL = 0, the same bytes as an explicit 0.  One host
   wait for the whole proof (the transcript stays on the device, like zk_gkr_prove); t is left intact */
int32_t zk_gprod_prove(zk_ctx *ctx, const zk_mle *t, const uint64_t *shift, const uint8_t seed[32], uint64_t out_product[4],
                       uint8_t *out_proof, uint64_t *out_point, uint64_t out_claim[4]);
/* no reference item; definition: tests/gprod_ref.py verify.
   host only, needs no context and no GPU: *out_ok = 1 / 0; out_point (n_vars elements) and out_claim are written only when *out_ok = 1.
   A proof element that is not canonical (>= p) makes *out_ok = 0, not an error */
int32_t zk_gprod_verify_host(int32_t field, uint32_t n_vars, const uint64_t *shift, const uint8_t seed[32], const uint64_t product[4],
                             const uint8_t *proof, uint64_t proof_len, uint64_t *out_point, uint64_t out_claim[4], int32_t *out_ok);
/* Errors of this section, in this order: a NULL pointer (but a NULL shift is legal) -> ZK_ERR_BAD_ARG; an unknown field ->
 * ZK_ERR_BAD_FIELD; a handle of another context -> ZK_ERR_CONTEXT_MISMATCH; n_vars == 0 or > 40, a shift or product that is not fully
 * reduced, proof_len != zk_gprod_proof_bytes -> ZK_ERR_BAD_ARG; a failed allocation -> ZK_ERR_ALLOC with nothing left behind.  On an
 * error nothing is written. */

/* ---- fractional-sum (LogUp) argument and lookup multiplicities (zk_amd/csrc/fsum.hip) ------------------------------
 * The reference has nothing like it; tests/fsum_ref.py defines every byte.  N / D = sum_i p[i] / (q[i] + shift) is shown to a verifier who is
 * left with TWO claims p(point) = claims[0], q(point) = claims[1], which the caller checks however it can (zk_mle_evaluate, or a
 * zk_mlpcs_open at that point): what a lookup argument is built on, with no committed helper inverses and no inversion in the prover.
 * Tree: P_n = p (all ones when p is NULL), Q_n = q + shift; P_j[i] = P_{j+1}[i] Q_{j+1}[i + 2^j] + P_{j+1}[i + 2^j] Q_{j+1}[i], Q_j[i] =
 * Q_{j+1}[i] Q_{j+1}[i + 2^j] (variable 0 = the index's top bit); N = P_0[0], D = Q_0[0].  Layer j = 0 .. n - 1 turns the claims on level j
 * into claims on level j + 1 by a sumcheck of eq(x, r_j) [P0 Q1 + P1 Q0 + lambda_j Q0 Q1](x) (degree 3, j rounds) and the four values p0,
 * p1, q0, q1 at its point; proof = per layer the 4 j round evaluations, then the four values: 2 n^2 + 2 n elements as 32-byte big-endian
 * canonical integers.  sum = [N | D] (4 limbs each), claims = [p(point) | q(point)].  A zero denominator is no error of the tree or the
 * prover (D = 0); the verifier rejects D = 0.
 * BINDING: the argument does NOT absorb the tables: the 32-byte seed must bind them, e.g. the roots of their commitments; a shift drawn as
 * a challenge must be drawn after that.  A lookup made of two such sums is sound only when the witness has fewer entries than the
 * field's characteristic, and its multiplicities must be committed and bound by the seed before the shift is drawn. */
/* no reference item; definition: tests/fsum_ref.py fraction_tree.
   *out_p, *out_q = two new tables of n_vars variables in heap order: out[2^j + i] = level j for 0 <= j < n_vars, out_p[0] = 0, out_q[0] = 1
   (so out_p[1] = N, out_q[1] = D; out_q is zk_mle_product_tree's heap of q, bit for bit); p NULL = all ones, shift NULL = 0.
   Stream-ordered, no host wait; p and q are left intact */
int32_t zk_mle_fraction_tree(zk_ctx *ctx, const zk_mle *p, const zk_mle *q, const uint64_t *shift, zk_mle **out_p, zk_mle **out_q);
/* 64 n_vars (n_vars + 1) */
int32_t zk_fsum_proof_bytes(uint32_t n_vars, uint64_t *out);
/* no reference item; definition: tests/fsum_ref.py prove.
   out_sum = [N | D], out_proof = zk_fsum_proof_bytes(n_vars) bytes; out_point (n_vars elements) and out_claims are what the verifier will
   derive.  p NULL = all ones (the verifier then checks that claim itself), shift NULL = 0, the same bytes as an explicit 0.  One host
   wait for the whole proof; p and q are left intact */
int32_t zk_fsum_prove(zk_ctx *ctx, const zk_mle *p, const zk_mle *q, const uint64_t *shift, const uint8_t seed[32], uint64_t out_sum[8],
                      uint8_t *out_proof, uint64_t *out_point, uint64_t out_claims[8]);
/* no reference item; definition: tests/fsum_ref.py verify.
   host only, needs no context and no GPU: *out_ok = 1 / 0; out_point (n_vars elements) and out_claims are written only when *out_ok = 1.
   has_p = 0: the proof was made with p = NULL, and claims[0] = 1 is checked here.  D = 0, or a proof element that is not canonical
   (>= p), makes *out_ok = 0, not an error */
int32_t zk_fsum_verify_host(int32_t field, uint32_t n_vars, int32_t has_p, const uint64_t *shift, const uint8_t seed[32], const uint64_t sum[8],
                            const uint8_t *proof, uint64_t proof_len, uint64_t *out_point, uint64_t out_claims[8], int32_t *out_ok);
/* no reference item; definition: tests/fsum_ref.py multiplicities.
   *out_m = a new table of the table's n_vars: m[j] = #{i : witness[i] = table[j]} as a field element if j is the lowest index holding
   that value, else 0; *out_missing = the witness entries found nowhere in the table, *out_first_missing the lowest such index (2^64 - 1:
   none), *out_duplicates = 2^n_vars - the number of distinct table values.  Any table of 0 .. 30 and witness of 0 .. 31 variables (above:
   ZK_ERR_UNSUPPORTED).  The result does not depend on the order in which threads arrive.  One host wait, for the three counters; the
   table m is stream-ordered; both inputs are left intact */
int32_t zk_lookup_multiplicities(zk_ctx *ctx, const zk_mle *table, const zk_mle *witness, zk_mle **out_m, uint64_t *out_missing,
                                 uint64_t *out_first_missing, uint64_t *out_duplicates);
/* Errors of this section, in this order: a NULL pointer (but a NULL p and a NULL shift are legal) -> ZK_ERR_BAD_ARG; an unknown field ->
 * ZK_ERR_BAD_FIELD; a handle of another context -> ZK_ERR_CONTEXT_MISMATCH; n_vars == 0 or > 40, p and q of different n_vars, a shift or
 * sum element that is not fully reduced, proof_len != zk_fsum_proof_bytes -> ZK_ERR_BAD_ARG; a failed allocation -> ZK_ERR_ALLOC with
 * nothing left behind.  On an error nothing is written. */

/* ---- zerocheck argument: a custom gate over k columns holds on every row (zk_amd/csrc/zerocheck.hip) --------------
 * The reference has nothing like it; tests/zerocheck_ref.py defines every byte.  Gate: G(x_0 .. x_{k-1}) = sum_{i < T} c_i prod_{f in term
 * i} x_f -- a term is a list of column indices (a repeat is a power, the empty term a constant; a column may appear in any number of
 * terms, or in none), its degree d the longest term.  Limits: 1 <= k <= 16, 1 <= T <= 32, 1 <= d <= 6, at most 64 factor mentions in all
 * (vanilla Plonk, qL a + qR b + qM a b + qO c + qC: k = 8, T = 5, d = 3).  Statement: G(t_0[i], .., t_{k-1}[i]) = 0 for every i < 2^n
 * (variable 0 = the index's top bit), shown to a verifier who is left with k claims t_c(point) = claims[c] at ONE point, which is what
 * zk_mlbatch_open takes.  Transcript: the seed; be64 of the field id, n, k, T; per term be32(c_i), be64(length), be64 per factor; then
 * tau_0 .. tau_{n-1} are drawn.  Round j = 0 .. n - 1 sends the eq-factored message g_j(X) = sum_{x'} eq(x', (tau_{j+1} ..)) G(T_j(X,
 * x')) at X = 0 .. d (the factors eq(tau_{<j}, rho_{<j}) and eq(tau_j, X) are not in it), rho_j is drawn and every column is folded at it;
 * at the end the k values v_c = t_c(rho) are absorbed.  The verifier starts from e_0 = 0, checks (1 - tau_j) g_j(0) + tau_j g_j(1) = e_j,
 * takes e_{j+1} = g_j(rho_j) by interpolation on 0 .. d, and at the end checks G(v) = e_n.  Proof = n (d + 1) + k elements as 32-byte
 * big-endian canonical integers.  The prover does not check the statement: on tables that violate the gate it makes the definition's
 * bytes, and the verifier rejects them.
 * BINDING: the argument does NOT absorb the tables (prove_partial does not either): the 32-byte seed must bind them, e.g. the root of
 * the tables' batch commitment. */
typedef struct zk_gate zk_gate;   /* a gate: a host object, no context */
/* coeffs: n_terms x 4 Montgomery limbs; term_len: n_terms lengths; factors: the terms' column indices, flat, term after term */
int32_t zk_gate_create(int32_t field, uint32_t k, uint32_t n_terms, const uint64_t *coeffs, const uint32_t *term_len, const uint32_t *factors,
                       zk_gate **out);
int32_t zk_gate_free(zk_gate *gate);
int32_t zk_gate_degree(const zk_gate *gate, uint32_t *out);
int32_t zk_gate_n_columns(const zk_gate *gate, uint32_t *out);
/* 32 (n_vars (d + 1) + k) */
int32_t zk_zerocheck_proof_bytes(const zk_gate *gate, uint32_t n_vars, uint64_t *out);
/* no reference item; definition: tests/zerocheck_ref.py prove.
   tables: the gate's k columns, all of one n_vars; out_proof = zk_zerocheck_proof_bytes bytes; out_point (n_vars elements) and out_claims
   (k elements) are what the verifier will derive.  One host wait for the whole proof (the transcript stays on the device, like
   zk_gprod_prove); the tables are left intact */
int32_t zk_zerocheck_prove(zk_ctx *ctx, const zk_mle *const *tables, const zk_gate *gate, const uint8_t seed[32], uint8_t *out_proof,
                           uint64_t *out_point, uint64_t *out_claims);
/* no reference item; definition: tests/zerocheck_ref.py verify.
   host only, needs no context and no GPU, and nothing sized by 2^n_vars: *out_ok = 1 / 0; out_point (n_vars elements) and out_claims (k
   elements) are written only when *out_ok = 1.  A proof element that is not canonical (>= p) makes *out_ok = 0, not an error */
int32_t zk_zerocheck_verify_host(const zk_gate *gate, uint32_t n_vars, const uint8_t seed[32], const uint8_t *proof, uint64_t proof_len,
                                 uint64_t *out_point, uint64_t *out_claims, int32_t *out_ok);
/* no reference item; definition: tests/zerocheck_ref.py gate_sums.
   out[X] = sum_{x' < 2^(n_vars - 1)} eq(x', tail) G(T(X, x')), X = 0 .. d (d + 1 elements), of the tables as they are: the round kernel
   without its fold, public in its own right as zk_mle_eq_sums is.  tail: n_vars - 1 elements, may be NULL for n_vars = 1.  Waits for the
   stream; the tables are left intact */
int32_t zk_mle_gate_sums(zk_ctx *ctx, const zk_mle *const *tables, const zk_gate *gate, const uint64_t *tail, uint64_t *out);
/* Errors of this section, in this order: a NULL pointer (a NULL table among them; but a NULL tail is legal for n_vars = 1) ->
 * ZK_ERR_BAD_ARG; an unknown field -> ZK_ERR_BAD_FIELD; a table of another context -> ZK_ERR_CONTEXT_MISMATCH; k, n_terms, a term's
 * length or the mentions outside the limits, a factor >= k, a coefficient or tail element that is not fully reduced, d = 0, tables of
 * different n_vars, n_vars == 0 or > 40, a gate of another field than the context's, proof_len != zk_zerocheck_proof_bytes ->
 * ZK_ERR_BAD_ARG; a failed allocation -> ZK_ERR_ALLOC with nothing left behind.  On an error nothing is written. */

/* ---- wiring (copy-constraint) permutation argument over k columns (zk_amd/csrc/perm.hip) ----------------------------
 * The reference has nothing like it; tests/perm_ref.py defines every byte, on top of tests/gprod_ref.py.  k witness columns w_c and k
 * permutation columns sigma_c (1 <= k <= 16), all of n variables (variable 0 = the index's top bit).  Cell (c, i) has the label c 2^n + i,
 * and sigma_c[i] is the label of the cell that (c, i) is wired to, as a field element.  Statement: w(sigma(cell)) = w(cell) for every cell,
 * shown to a verifier who is left with 2 k claims w_c(point) = claims[c], sigma_c(point) = claims[k + c] at ONE point of n elements, which
 * is what zk_mlbatch_open takes (together with a zerocheck's claims: one opening at two points).  K = 2^kappa is the next power of two
 * >= k, N = n + kappa + 1 <= 40.  Fingerprint table F of N variables, the side bit the LOWEST index bit: for v = c 2^n + i and c < k,
 * F[2v] = w_c[i] + beta v + gamma (identity side) and F[2v + 1] = w_c[i] + beta sigma_c[i] + gamma (sigma side); for k <= c < K both are
 * 1.  The product tree takes the top index bit away first, so its level 1 is the pair (identity side's product, sigma side's product).
 * Proof: the grand-product proof of F with a NULL shift under seed' = Keccak-256(seed | be64 of the field id, n, k | be32(beta) |
 * be32(gamma)), byte for byte what zk_gprod_prove makes on F with seed'; then the 2 k values w_c(r_lo), sigma_c(r_lo): 2 N^2 + 2 k
 * elements as 32-byte big-endian canonical integers.  No product is sent.  Verifier: a, b = the first two elements; a == b; the
 * grand-product verifier with the product a b; its point splits into r_hi (kappa elements), r_lo (n) and r_s; accept iff its claim equals
 * sum_{c<k} eq(r_hi, c) (vw_c + beta ((1 - r_s) (c 2^n + sum_b r_lo[b] 2^(n-1-b)) + r_s vs_c) + gamma) + sum_{k<=c<K} eq(r_hi, c).  The
 * prover does not check the statement: on broken wiring it makes the definition's bytes, and the verifier rejects them.
 * BINDING: the argument does NOT absorb the tables: the 32-byte seed must bind the commitments of w and sigma (the root of their batch
 * commitment), and beta, gamma must be drawn after that.  That sigma is a permutation of the labels is the circuit's preprocessing to
 * guarantee; the argument does not check it. */
/* 32 (2 N^2 + 2 k) */
int32_t zk_perm_proof_bytes(uint32_t n_vars, uint32_t k, uint64_t *out);
/* no reference item; definition: tests/perm_ref.py fingerprint.
   *out = F as a new table of N variables.  Stream-ordered, no host wait, public in its own right as zk_mle_product_tree is; the columns
   are left intact */
int32_t zk_mle_perm_fingerprint(zk_ctx *ctx, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, const uint64_t beta[4],
                                const uint64_t gamma[4], zk_mle **out);
/* no reference item; definition: tests/perm_ref.py prove.
   out_proof = zk_perm_proof_bytes(n_vars, k) bytes; out_point (n_vars elements) and out_claims (2 k elements: the w values, then the
   sigma values) are what the verifier will derive.  F is made on the device and never leaves it (k_perm_leaves, then the product tree's
   launches; ZK_PERM_FUSE=1 joins F to the tree's first launch).  TWO host waits: one for the grand product's block, whose point picks the point of
   the end values, one for the 2 k values (zk_mle_evaluate's launches).  The columns are left intact */
int32_t zk_perm_prove(zk_ctx *ctx, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, const uint64_t beta[4], const uint64_t gamma[4],
                      const uint8_t seed[32], uint8_t *out_proof, uint64_t *out_point, uint64_t *out_claims);
/* no reference item; definition: tests/perm_ref.py verify.
   host only, needs no context and no GPU, and nothing sized by 2^n_vars: *out_ok = 1 / 0; out_point (n_vars elements) and out_claims
   (2 k elements) are written only when *out_ok = 1.  A proof element that is not canonical (>= p) makes *out_ok = 0, not an error */
int32_t zk_perm_verify_host(int32_t field, uint32_t n_vars, uint32_t k, const uint64_t beta[4], const uint64_t gamma[4], const uint8_t seed[32],
                            const uint8_t *proof, uint64_t proof_len, uint64_t *out_point, uint64_t *out_claims, int32_t *out_ok);
/* Errors of this section, in this order: a NULL pointer (a NULL table in the arrays among them) -> ZK_ERR_BAD_ARG; an unknown field ->
 * ZK_ERR_BAD_FIELD; a table of another context -> ZK_ERR_CONTEXT_MISMATCH; k outside 1..16, columns of different n_vars, n_vars == 0 or
 * N > 40, a beta or gamma that is not fully reduced, proof_len != zk_perm_proof_bytes -> ZK_ERR_BAD_ARG; a failed allocation ->
 * ZK_ERR_ALLOC with nothing left behind.  On an error nothing is written. */

/* ---- measurement hooks (bench.py) ------------------------------------------------------------------------------ */
/* time `reps` launches of the MSB fold of `t` into `out` with HIP events on the context's stream; average ms/launch */
int32_t zk_bench_fold(zk_ctx *ctx, const zk_mle *t, const uint64_t r[4], zk_mle *out, int32_t reps, double *out_ms);
/* the same with one event every `group` launches: out_ms_each[i] = average launch duration inside group i,
   ceil(reps / group) values (at most 65536); group = 1 brackets every launch (an event record costs the stream ~4 us) */
int32_t zk_bench_fold_samples(zk_ctx *ctx, const zk_mle *t, const uint64_t r[4], zk_mle *out, int32_t reps, int32_t group,
                              double *out_ms_each);
/* the same for zk_ntt (all passes of one transform), average ms per transform */
int32_t zk_bench_ntt(zk_ctx *ctx, const zk_mle *in, int32_t inverse, zk_mle *out, int32_t reps, double *out_ms);
/* zk_upoly_interpolate (xs NULL) or zk_upoly_interpolate_xy (xs of n points, ys at least n long, every x distinct) of n points,
   `reps` times: out_ms[0..5) = average ms of the call, its weights, direct tree levels, NTT tree levels and block merges */
int32_t zk_bench_upoly_interp(zk_ctx *ctx, const zk_upoly *xs, const zk_upoly *ys, int32_t reps, double *out_ms);
/* zk_upoly_evaluate_many of p (not empty) at xs (not empty), `reps` times after one untimed run, on path 0 (the model / the switch),
   1 (direct) or 2 (tree; ZK_ERR_UNSUPPORTED where it is not available): out_ms[0..6) = average ms of the call and, on the tree path,
   of its up-sweep, series inversion, root vector, NTT levels of the down-sweep and bottom kernel (zeros on the direct path) */
int32_t zk_bench_upoly_evaluate_many(zk_ctx *ctx, const zk_upoly *p, const zk_upoly *xs, int32_t path, int32_t reps, double *out_ms);
/* zk_upoly_divrem of a by b (la >= lb >= 1, b's leading coefficient not zero), both results, `reps` times after one untimed run, on
   path 0 (the switches), 1 (direct), 2 (linear) or 3 (Newton); a path that is not available for the shape -> ZK_ERR_BAD_ARG:
   out_ms[0..4) = average ms of the call and, on the Newton path, of its series inverse, quotient product and remainder (zeros on
   the other paths) */
int32_t zk_bench_upoly_divrem(zk_ctx *ctx, const zk_upoly *a, const zk_upoly *b, int32_t path, int32_t reps, double *out_ms);
/* device time of the dense coefficient-form calls, `reps` back-to-back enqueues between two HIP events, average ms per call:
   op 0 = zk_cmle_interpolate of t, op 1 = zk_cmle_to_evaluation of p, op 2 = zk_cmle_evaluate of p at point (its launches; the host
   arithmetic between them included, the final wait not) */
int32_t zk_bench_cmle(zk_ctx *ctx, int32_t op, const zk_mle *t, const zk_cmle *p, const uint64_t *point, uint64_t n_point, int32_t reps,
                      double *out_ms);
/* the same for the algebra calls (each rep is the whole call, its result handed straight back to the pool): op 0 =
   zk_cmle_partial_evaluate of a with the given assignments, 1 = zk_cmle_add(a, b), 2 = zk_cmle_scalar_multiply of a by values[0..4),
   3 = zk_cmle_mul(a, b) (tools/cmle_algebra_bench.py) */
int32_t zk_bench_cmle_algebra(zk_ctx *ctx, int32_t op, const zk_cmle *a, const zk_cmle *b, const uint8_t *selectors,
                              const uint64_t *selector_lens, const uint64_t *values, uint64_t n_assign, int32_t reps, double *out_ms);
/* device time of `reps` zk_mle_batch_inverse calls (shift 0, no count) of t into out by HIP events after as many untimed ones, average
   ms per call, like the other zk_bench_* hooks: path 0 = the default (the switch), 1 = the one-launch kernel (a table of more than one
   chunk -> ZK_ERR_UNSUPPORTED), 2 = the three launches, 3 = zk_mle_prefix_product (exclusive) of t into out; another path, reps < 1
   or a NULL -> ZK_ERR_BAD_ARG (tools/batch_inverse_bench.py) */
int32_t zk_bench_batch_inverse(zk_ctx *ctx, const zk_mle *t, zk_mle *out, int32_t path, int32_t reps, double *out_ms);
/* device time of `reps` builds of the whole tree over the columns (into a tree of the hook's own) by HIP events after as many untimed
   ones, average ms per build, like the other zk_bench_* hooks: path 0 = the default (the switch), 1 = the fused sub-tree stages, 2 = one
   launch per level; another path, reps < 1 or a NULL -> ZK_ERR_BAD_ARG, then the errors of zk_merkle_commit (tools/merkle_bench.py) */
int32_t zk_bench_merkle(zk_ctx *ctx, const zk_mle *const *columns, uint32_t n_columns, int32_t path, int32_t reps, double *out_ms);
/* device time of `reps` folds of `in` by 2^log_arity into `out` (shift and challenge: fixed non-zero elements) by HIP events after as many
   untimed ones, average ms per fold; the power table and the binary path's intermediate layers are made once, outside the timed loop:
   path 0 = the default (the switch), 1 = the fused kernel, 2 = log_arity binary launches; another path, reps < 1 or a NULL ->
   ZK_ERR_BAD_ARG, then the errors of zk_fri_fold (tools/fri_bench.py) */
int32_t zk_bench_fri_fold(zk_ctx *ctx, const zk_mle *in, uint32_t log_arity, zk_mle *out, int32_t path, int32_t reps, double *out_ms);
/* device time of `reps` zk_deep_quotient launches of the columns into `out` (shift, z, alpha and values: fixed elements, z off the domain)
   by HIP events after as many untimed ones, average ms per quotient; the power table and the pointer array are made once, outside the
   timed loop: reps < 1 or a NULL -> ZK_ERR_BAD_ARG, then the errors of zk_deep_quotient (tools/pcs_bench.py) */
int32_t zk_bench_deep_quotient(zk_ctx *ctx, const zk_mle *const *columns, uint32_t n_columns, zk_mle *out, int32_t reps, double *out_ms);
/* device time of the sumcheck side of `reps` zk_mlpcs_open calls on the table t (all n_vars rounds with a fixed point and fixed
   challenges: the eq factors, round 0's sums, then per round the fold of T joined to its sums; no transcript, no host wait) by HIP events
   after as many untimed ones, average ms per opening: path 0 = the default (the switch), 1 = the fused round kernel, 2 = the eq table
   with two-table round sums and two folds per round; another path, reps < 1 or a NULL -> ZK_ERR_BAD_ARG.  t is left intact
   (tools/mlpcs_bench.py) */
int32_t zk_bench_mlpcs_round(zk_ctx *ctx, const zk_mle *t, int32_t path, int32_t reps, double *out_ms);
/* device time of `reps` runs on the handle's tables by HIP events after as many untimed ones, average ms per run: path 0 = the device
   work of one zk_mlbatch_open at n_points points on the default route (the values' sums, T_0, every round's fold, tree and sums, the
   final transform; fixed challenges, no transcript, no host wait, no gather), 1 = k_ml_combine_fold alone, 2 = its unfused counterpart
   (zk_mle_lincomb's launch into a scratch layer, then FRI's fold), 3 = one round (fold joined to the sums) at kMlPointsPerPass points
   in one pass over the first table, 4 = the same as kMlPointsPerPass single-point passes; n_points is read by path 0 only (1..16);
   another path, reps < 1 or a NULL -> ZK_ERR_BAD_ARG.  The handle is left intact (tools/mlbatch_bench.py) */
int32_t zk_bench_mlbatch(zk_ctx *ctx, const zk_mlbatch *h, uint32_t n_points, int32_t path, int32_t reps, double *out_ms);
/* device time of `reps` runs on the table t by HIP events after as many untimed ones, average ms per run, like the other zk_bench_*
   hooks: path 0 = zk_mle_product_tree's launches on the default route (the switch), 1 = the same with one level per launch above the
   one-workgroup LDS stage, 2 = the whole proof as zk_gprod_prove enqueues it (no shift, a fixed seed: the tree, every layer's eq table,
   sumcheck and transcript step; without the proof block's way to the host and its one wait); another path, reps < 1 or a NULL ->
   ZK_ERR_BAD_ARG, then the errors of zk_gprod_prove.  t is left intact (tools/gprod_bench.py) */
int32_t zk_bench_gprod(zk_ctx *ctx, const zk_mle *t, int32_t path, int32_t reps, double *out_ms);
/* device time of `reps` runs on the table q by HIP events after as many untimed ones, average ms per run: path 0 = zk_mle_fraction_tree's
   launches on the default route with p = ones (the switch), 1 = the same with one level per launch above the one-workgroup LDS stage, 2 =
   the whole proof as zk_fsum_prove enqueues it (p = ones, no shift, a fixed seed; without the proof block's way to the host and its one
   wait), 3 = zk_lookup_multiplicities' launches with the witness equal to the table q; another path, reps < 1 or a NULL ->
   ZK_ERR_BAD_ARG, then the errors of zk_fsum_prove.  q is left intact (tools/fsum_bench.py) */
int32_t zk_bench_fsum(zk_ctx *ctx, const zk_mle *q, int32_t path, int32_t reps, double *out_ms);
/* device time of `reps` runs on the gate's k tables by HIP events after as many untimed ones, average ms per run: path 0 = the whole
   proof as zk_zerocheck_prove enqueues it (a fixed seed; without the proof block's way to the host and its one wait), 1 = the round-0
   launch alone (k_zc_round without a fold), 2 = the round-1 launch alone, the fold at rho_0 joined to the sums (n_vars >= 2); the gate
   program, tau's tables and rho_0 are made once, outside the timed loop; another path, reps < 1 or a NULL -> ZK_ERR_BAD_ARG, then the
   errors of zk_zerocheck_prove.  The tables are left intact (tools/zerocheck_bench.py) */
int32_t zk_bench_zerocheck(zk_ctx *ctx, const zk_mle *const *tables, const zk_gate *gate, int32_t path, int32_t reps, double *out_ms);
/* device time of `reps` runs on the k + k columns by HIP events after as many untimed ones, average ms per run: path 0 = F and the whole
   product tree over it on the default route (the switches), 1 = the same on the unfused route (k_perm_leaves, then
   zk_mle_product_tree's launches over F), 3 = on the fused route (k_perm_tree, then the tree's other launches), 2 = the whole proof as
   zk_perm_prove enqueues it (beta = 2, gamma = 1, a fixed seed, the 2 k evaluations at a fixed point; without the two ways to the host
   and their waits); another path, reps < 1 or a
   NULL -> ZK_ERR_BAD_ARG, then the errors of zk_perm_prove.  The columns are left intact (tools/perm_bench.py) */
int32_t zk_bench_perm(zk_ctx *ctx, const zk_mle *const *w, const zk_mle *const *sigma, uint32_t k, int32_t path, int32_t reps, double *out_ms);
/* wall clock of `reps` zk_sumcheck_prove calls (prove_partial semantics: absorb_table = 0, the tables are left intact), each
   measured around the whole call with std::chrono -- every launch, the transcript, the download of the proof and the one host
   wait -- as SURVEY 8(d) prescribes for the prover; out_ms_each[reps].  What a compiled host sees: no binding overhead. */
int32_t zk_bench_prove_partial(zk_ctx *ctx, zk_mle *const *factors, uint64_t k, uint32_t max_var_degree, const uint64_t sum[4],
                               int32_t reps, double *out_ms_each);
/* the same for zk_mle_evaluate (the reference's own criterion bench, polynomial/benches/polynomial_evaluation.rs): per-call ms */
int32_t zk_bench_evaluate(zk_ctx *ctx, const zk_mle *t, const uint64_t *point, uint64_t n_point, int32_t reps, double *out_ms_each);
/* device time of the same call: `reps` back-to-back enqueues of evaluate's launches between two HIP events on the context's stream,
   no host wait in between; average ms per evaluate (bench.py roofline_evaluate) */
int32_t zk_bench_evaluate_device(zk_ctx *ctx, const zk_mle *t, const uint64_t *point, uint64_t n_point, int32_t reps, double *out_ms);
/* register-resident modular-multiply throughput (no memory traffic): variant 0 = fe_mul chain. Returns modmul/s */
int32_t zk_bench_modmul(zk_ctx *ctx, int32_t variant, int32_t iters, double *out_modmul_per_s);
/* plain 16-B/lane streaming copy of `bytes` bytes: achieved GB/s (calibrates the HBM ceiling on this device) */
int32_t zk_bench_copy(zk_ctx *ctx, uint64_t bytes, int32_t reps, double *out_gbps);

/* ---- environment switches (zk_amd/csrc/env.hpp) ------------------------------------------------------------------
   Read once per process; every one is a tuning / A-B / debug override and every setting produces bit-identical results.  A value
   that is not a whole decimal number inside the accepted range is ignored (the default applies) with one line on stderr.

   name                    default   accepted     meaning
   ZK_SKIP1_MIN_PAIRS      65536     1 .. 2^40    rounds with at least this many pairs leave S(1) to the tail (S(1) = claim - S(0))
   ZK_LEAD_MIN_PAIRS       65536     1 .. 2^40    ... accumulate the leading coefficient instead of S(D) (K = D shapes)
   ZK_QUAD_MAX_PAIRS       32768     0 .. 2^40    rounds up to this size run four lanes per pair index (k_round_quad); 0 = never
   ZK_PIPE_MAX_PAIRS       4096      0 .. 2^40    rounds up to this size are prepared before their challenge exists; 0 = never
   ZK_ROUND_MIN_BLOCKS     512 / 256 1 .. 2048    smallest grid of the fused round kernels (256 for the GKR shape)
   ZK_FINISH_PIPE          1         0 .. 1       0: the classic single-workgroup finisher instead of the pipelined one
   ZK_SPONGE_IN_TAIL       1         0 .. 1       0: the initial sponge state goes to the device with a launch of its own instead of as an argument of round 0's tail
   ZK_ROUND0_DOT29         1         0 .. 2       0: round 0 of the two-table degree-2 shapes on the wide accumulator; 2: force dot29
   ZK_ROUND_GLDS           1         0 .. 1       0: the big rounds on k_round0_dot29 / k_round_kd instead of the LDS-DMA kernels (k_round0_glds, k_round_fused_glds)
   ZK_ROUND_GLDS_MIN_PAIRS per kernel 64 .. 2^40  smallest round (pairs, a multiple of 64) on the LDS-DMA kernels; unset: 2^21 / 2^20 (round 0: 2 tables / 2 + term), 2^16 / 2^19 (fused: 3 tables / 2 + term)
   ZK_ROUND_GLDS_NT_MIN_PAIRS 2^20   64 .. 2^40   fused LDS-DMA rounds at least this big store their half tables nontemporal
   ZK_EVAL_FOLDS           off       flag         variable-by-variable evaluate (one fold launch per variable)
   ZK_EVAL_STREAM_MIN      21        0 .. 1000    smallest table (variables) that takes the streaming evaluate kernel
   ZK_EVAL_STREAM_LEAVE    8 / 9     7 .. 12      variables the streaming launch leaves (log2 of its grid): 8 at 21 variables, 9 above
   ZK_EVAL_WEIGHT          3         0 .. 3       bit 0 / bit 1: k_eval_low / k_eval_stream weight their outputs (no second bulk launch)
   ZK_ZETA_GLOBAL          off       flag         to_evaluation_form by global passes of three index bits (round 4's path)
   ZK_ZETA_DEVICE_SORT_MIN 4096      0 .. 2^40    to_evaluation_form: term lists at least this long are ordered on the device (0: always)
   ZK_NTT_FULL_TABLE_MAX_LOG 24      0 .. 24      largest inter-pass twiddle table (log2 entries) kept in HBM; smaller: composed per element (slower, less traffic)
   ZK_UPOLY_DIRECT_MAX     model     0 .. 2^40    zk_upoly_mul: set, products whose shorter operand has at most this many coefficients take the direct convolution, the
                                                  others the NTT; unset, a cost model fitted to the measured crossover (below 2^8 points always direct)
   ZK_UPOLY_INTERP_DIRECT_LOG 7   7 .. 8       zk_upoly_interpolate(_xy): subproduct-tree nodes of up to 2^this points are built by the direct LDS kernel, larger ones by
                                                  batched NTT levels (measured crossover, profiles/upoly_interp.log)
   ZK_UPOLY_EVALMANY_DIRECT_MAX model 0 .. 2^40 zk_upoly_evaluate_many: set, shapes with n * len(p) at most this take the direct kernel, the others the transposed tree
                                                  (0: always the tree where its length rule allows it); unset, a cost model fitted to profiles/upoly_evalmany.log (n = L: direct up to 2^14)
   ZK_UPOLY_INTERP_XY_TREE_MIN 16384 1 .. 2^40      zk_upoly_interpolate_xy: from this many points on the weights' denominators come from the multipoint evaluation's tree
                                                  path, below it from the O(nx m) kernel (measured crossover: 2^14 8.1 ms against 13.9, 2^12 6.0 against 4.8; profiles/upoly_evalmany.log)
   ZK_UPOLY_DIVREM_DIRECT_MAX 1023  0 .. 2^40    zk_upoly_divrem: dividends of at most this many coefficients take the one-workgroup schoolbook kernel (values above 2048, its
                                                  LDS limit, count as 2048; 0: never).  Measured at la = 2 lb (profiles/upoly_divrem.log): 2^9 1.25 ms against Newton's 1.27,
                                                  2^10 2.22 against 1.54 -- from 2^10, the smallest measured size at which Newton wins, the default leaves it to Newton
   ZK_UPOLY_DIVREM_LINEAR  1         0 .. 1       zk_upoly_divrem: 0 sends divisors of two coefficients to the other paths instead of the affine scan
   ZK_BATCH_INV_ONE_LAUNCH_MAX 2048  0 .. 2048    zk_*_batch_inverse: lengths up to this run in one launch of one workgroup (one chunk at most), longer ones in three
                                                  launches; 0: always three (profiles/batch_inverse.log has both sides)
   ZK_MERKLE_FUSE_LEVELS   0         0 .. 10      zk_merkle_commit: 0 builds the tree with one launch per level; s > 0 with fused stages in which a workgroup climbs s levels
                                                  over a tile of 2^s digests in LDS, and one workgroup finishes the last 6 levels (profiles/merkle.log has both sides)
   ZK_FRI_FUSED_FOLD       1         0 .. 1       zk_fri_fold / zk_fri_prove: 1 folds by 2^a in one launch with the a butterfly levels in registers; 0 in a binary
                                                  launches through intermediate layers (profiles/fri.log has both sides)
   ZK_MLPCS_ROUND          1         0 .. 1       zk_mlpcs_open: 1 runs the sumcheck side on the fused round kernel (no eq table, the fold of T joined to the round's two
                                                  sums); 0 on zk_eq_table with two-table round sums and two folds per round (profiles/mlpcs.log has both sides)
   ZK_MLBATCH_FUSE_FOLD    1         0 .. 1       zk_mlbatch_open: 1 combines the k codewords and folds them in one pass (k_ml_combine_fold: the combined layer 0 is never
                                                  written); 0 writes it with zk_mle_lincomb's kernel and folds it with FRI's (profiles/mlbatch.log has both sides)
   ZK_GPROD_TREE_FUSE      0         0 .. 3       zk_mle_product_tree / zk_gprod_prove: levels of the product tree per launch above the one-workgroup LDS stage
                                                  (k_ptree<1..3>); 0 = the default, 3 (profiles/gprod.log has both ends)
   ZK_PERM_FUSE            0         0 .. 1       zk_perm_prove: 0 writes the fingerprint table with k_perm_leaves and runs the product tree over it; 1 writes it and the first
                                                  levels of the tree in one launch (k_perm_tree<1..2>, the arity by ZK_GPROD_TREE_FUSE, at most 2), which measures
                                                  slower: 0.67 to 0.75 ms against 0.50 at N = 24 (profiles/perm.log has both sides)
   ZK_PERM_MAX_GRID        16384     1 .. 16384   zk_perm_prove under ZK_PERM_FUSE=1: the largest grid of k_perm_tree, whose waves loop over their runs above it (a small value sends a small
                                                  shape round the loop: tests)
   ZK_FSUM_TREE_FUSE       0         0 .. 2       zk_mle_fraction_tree / zk_fsum_prove: levels of the fraction tree per launch above the one-workgroup LDS stage
                                                  (k_ftree<1..2>; three levels do not fit the registers); 0 = the default, 2 (profiles/fsum.log has both ends)
   ZK_TO_BYTES_THREADS     affinity  1 .. 4       host threads copying to_bytes chunks to the caller / gathering zk_mle_upload_shard's shard (default: CPUs allowed, at most 4)
   ZK_PUBLISH_IN_FINISHER  1         0 .. 1       0: the proof block always goes to pinned host memory by a launch of its own (k_publish_host)
   ZK_CLAIM_IN_ROUND       1         0 .. 1       0: the tails evaluate the SKIP1 claim S_prev(r_prev) themselves instead of reading it from the round kernel's claim workgroup
   ZK_SHARD_SKIP1          1         0 .. 1       0: the sharded prover's round kernels form every sum (no S(1) / S(D) derivation behind the all-reduce)
   ZK_SHARD_FAKE_ALLREDUCE_US 0      0 .. 1000    measurement aid: every all-reduce of the sharded loop is followed by a spin of this many microseconds
                                                  on its stream (a one-rank communicator standing in for a node's latency)
   ZK_PIPE_DEBUG / ZK_HOST_DEBUG  off  flag       phase stamps of the pipelined rounds / host enqueue + wait times on stderr
   ZK_BATCH_DEBUG                 off  flag       zk_sumcheck_prove_batch: report on stderr every launch replayed proof by proof   */

#ifdef __cplusplus
}
#endif
#endif /* ZK_AMD_H */
