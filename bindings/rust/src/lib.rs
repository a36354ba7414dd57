//! zk-amd-shim — the reference's hot-path API (same names, same signatures, same `&'static str` errors) over the C ABI
//! of libzk_amd.so (`include/zk_amd.h`).  SOURCE ONLY: no Rust toolchain exists in the build image, so this file is the
//! documented binding a maintainer adds.  It is checked two ways without `rustc`: `tests/test_rust_shim_audit.py` parses
//! the `extern "C"` block below and compares every function's arity and parameter widths with `include/zk_amd.h`, and
//! `tests/cpp/test_reference_kats.cpp` runs the same call sequences through the C++ mirror (`zk_amd/host/zk.hpp`).
//!
//! Reference items mirrored (paths relative to the reference checkout):
//!   polynomial/src/multilinear/evaluation_form.rs:4-103  MultiLinearPolynomial<F>  (Clone, Debug, PartialEq)
//!   polynomial/src/multilinear/pairing_index.rs:2-9      index_pair
//!   polynomial/src/multilinear/pairing_index.rs:24-26    mask
//!   polynomial/src/product_poly.rs:6-88                  ProductPoly<F>            (Clone, Debug, PartialEq)
//!   sumcheck/src/prover.rs:9-73                          SumcheckProver<MAX_VAR_DEGREE, F>
//!   sumcheck/src/verifier.rs:9-41                        SumcheckVerifier<F>
//!   sumcheck/src/lib.rs:8-20                             SumcheckProof<F>, SubClaim<F>
//!   transcript/src/lib.rs:5-35                           Transcript
//!   fft/src/lib.rs:4-46                                  fft, ifft, fft_internal
//!   polynomial/src/univariate_poly.rs:7-40,186-209       UnivariatePolynomial<F> (new, coefficients, evaluate, Mul;
//!                                                        Clone, Debug, PartialEq)
//!   polynomial/src/multilinear/coefficient_form.rs:27-415 CoeffMultilinearPolynomial<F>, dense and device-resident (interpolate,
//!                                                        partial_evaluate, relabel, scalar_multiply, Add, Mul, evaluate_slice,
//!                                                        to_evaluation_form, to_bytes, coefficients)
//!
//! With this crate the four tests at sumcheck/src/lib.rs:53-122 read unchanged apart from their `use` lines
//! (`polynomial::…::MultiLinearPolynomial` / `ProductPoly`, `crate::prover::SumcheckProver`,
//! `crate::verifier::SumcheckVerifier` -> `zk_amd_shim::…`; those tests build their inputs with the reference's own
//! `CoeffMultilinearPolynomial::new(terms)`, which stays the reference's: the type of that name here holds dense key sets only).  The
//! reference's tests sit inside the `sumcheck` crate and read the private fields `subclaim.challenges` / `subclaim.sum`;
//! here those fields are `pub` for the same reason.
//!
//! `F` must be one of the 4-limb Montgomery fields libzk_amd knows; ark-ff's in-memory layout of
//! `Fp<MontBackend<_, 4>>` (4 LE u64 limbs, Montgomery form) IS the wire format, so `Vec<F>` is passed by pointer.
//!
//! Contexts: ONE `zk_ctx` per (thread, field), created on first use and shared by reference count — every table holds an
//! `Rc` of its context, so the context (stream, scratch, block pool) is destroyed exactly when the thread's cache entry
//! and the last table are gone.  `Rc` and raw pointers make every type here `!Send`/`!Sync`: a table cannot leave the
//! thread whose context owns it, which is the C ABI's threading rule.  Device: `ZK_AMD_DEVICE` (default 0).
use ark_ff::PrimeField;
use std::cell::{OnceCell, RefCell};
use std::fmt;
use std::marker::PhantomData;
use std::os::raw::c_char;
use std::rc::Rc;

#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_ctx { _opaque: [u8; 0] }
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_mle { _opaque: [u8; 0] }
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_transcript { _opaque: [u8; 0] }
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_circuit { _opaque: [u8; 0] }
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_upoly { _opaque: [u8; 0] }
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_cmle { _opaque: [u8; 0] }
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_merkle { _opaque: [u8; 0] }
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_pcs { _opaque: [u8; 0] }
#[repr(C)]
pub struct zk_mlpcs { _opaque: [u8; 0] }
#[repr(C)]
pub struct zk_mlbatch { _opaque: [u8; 0] }
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct zk_gate { _opaque: [u8; 0] }

const ZK_ERR_EMPTY_PRODUCT: i32 = -3;
const ZK_ERR_ARITY_MISMATCH: i32 = -4;
const ZK_ERR_BAD_ARG: i32 = -20;
const ZK_ERR_PANIC_INDEX: i32 = -5;
const ZK_ERR_FFT_NOT_POW2: i32 = -6;
const ZK_ERR_FFT_NO_ROOT: i32 = -7;
const ZK_ERR_VERIFY_SUM: i32 = -9;
const ZK_ERR_GKR_REJECT: i32 = -27;

/// The ABI revision this file was written against (`ZK_AMD_ABI_VERSION` in include/zk_amd.h); checked once per context.
const ZK_AMD_ABI_VERSION: i32 = 6;

extern "C" {
    fn zk_abi_version() -> i32;
    fn zk_strerror(status: i32) -> *const c_char;
    fn zk_ctx_create(field: i32, device: i32, out_ctx: *mut *mut zk_ctx) -> i32;
    fn zk_ctx_destroy(ctx: *mut zk_ctx) -> i32;
    fn zk_mle_upload(ctx: *mut zk_ctx, n_vars: u64, evals: *const u64, len: u64, out: *mut *mut zk_mle) -> i32;
    fn zk_mle_clone(ctx: *mut zk_ctx, t: *const zk_mle, out: *mut *mut zk_mle) -> i32;
    fn zk_mle_free(ctx: *mut zk_ctx, t: *mut zk_mle) -> i32;
    fn zk_mle_n_vars(t: *const zk_mle, out_n_vars: *mut u64) -> i32;
    fn zk_mle_download(ctx: *mut zk_ctx, t: *const zk_mle, out_evals: *mut u64) -> i32;
    fn zk_mle_equal(ctx: *mut zk_ctx, a: *const zk_mle, b: *const zk_mle, out_equal: *mut i32) -> i32;
    fn zk_mle_partial_evaluate(ctx: *mut zk_ctx, t: *const zk_mle, initial_var: u64, assignments: *const u64,
                               n_assign: u64, out: *mut *mut zk_mle) -> i32;
    fn zk_mle_evaluate(ctx: *mut zk_ctx, t: *const zk_mle, point: *const u64, n_point: u64, out: *mut u64) -> i32;
    fn zk_mle_to_bytes(ctx: *mut zk_ctx, t: *const zk_mle, out_bytes: *mut u8) -> i32;
    // sharding by index mod world (include/zk_amd.h; zk_mle_unshard needs a communicator, which this shim has no type for)
    fn zk_mle_upload_shard(ctx: *mut zk_ctx, n_vars: u64, evals: *const u64, len: u64, world: u32, rank: u32,
                           out: *mut *mut zk_mle) -> i32;
    fn zk_mle_split(ctx: *mut zk_ctx, t: *const zk_mle, world: u32, out_shards: *mut *mut zk_mle) -> i32;
    fn zk_mle_interleave(ctx: *mut zk_ctx, shards: *const *const zk_mle, world: u32, out: *mut *mut zk_mle) -> i32;
    // UnivariatePolynomial (polynomial/src/univariate_poly.rs)
    fn zk_upoly_upload(ctx: *mut zk_ctx, coeffs: *const u64, len: u64, out: *mut *mut zk_upoly) -> i32;
    fn zk_upoly_len(p: *const zk_upoly, out_len: *mut u64) -> i32;
    fn zk_upoly_download(ctx: *mut zk_ctx, p: *const zk_upoly, out_coeffs: *mut u64) -> i32;
    fn zk_upoly_free(ctx: *mut zk_ctx, p: *mut zk_upoly) -> i32;
    fn zk_upoly_mul(ctx: *mut zk_ctx, a: *const zk_upoly, b: *const zk_upoly, out: *mut *mut zk_upoly) -> i32;
    fn zk_upoly_evaluate(ctx: *mut zk_ctx, p: *const zk_upoly, x: *const u64, out: *mut u64) -> i32;
    fn zk_upoly_add(ctx: *mut zk_ctx, a: *const zk_upoly, b: *const zk_upoly, out: *mut *mut zk_upoly) -> i32;
    fn zk_upoly_interpolate(ctx: *mut zk_ctx, ys: *const zk_upoly, out: *mut *mut zk_upoly) -> i32;
    fn zk_upoly_interpolate_xy(ctx: *mut zk_ctx, xs: *const zk_upoly, ys: *const zk_upoly, out: *mut *mut zk_upoly) -> i32;
    fn zk_upoly_evaluate_many(ctx: *mut zk_ctx, p: *const zk_upoly, xs: *const zk_upoly, out: *mut *mut zk_upoly) -> i32;
    fn zk_upoly_divrem(ctx: *mut zk_ctx, a: *const zk_upoly, b: *const zk_upoly, out_q: *mut *mut zk_upoly, out_r: *mut *mut zk_upoly) -> i32;
    fn zk_upoly_inverse_series(ctx: *mut zk_ctx, f: *const zk_upoly, k: u64, out: *mut *mut zk_upoly) -> i32;
    // CoeffMultilinearPolynomial, dense (polynomial/src/multilinear/coefficient_form.rs)
    fn zk_cmle_upload(ctx: *mut zk_ctx, n_vars: u64, coeffs: *const u64, len: u64, out: *mut *mut zk_cmle) -> i32;
    fn zk_cmle_download(ctx: *mut zk_ctx, p: *const zk_cmle, out_coeffs: *mut u64) -> i32;
    fn zk_cmle_n_vars(p: *const zk_cmle, out: *mut u64) -> i32;
    fn zk_cmle_free(ctx: *mut zk_ctx, p: *mut zk_cmle) -> i32;
    fn zk_cmle_interpolate(ctx: *mut zk_ctx, values: *const zk_mle, out: *mut *mut zk_cmle) -> i32;
    fn zk_cmle_to_evaluation(ctx: *mut zk_ctx, p: *const zk_cmle, out: *mut *mut zk_mle) -> i32;
    fn zk_cmle_evaluate(ctx: *mut zk_ctx, p: *const zk_cmle, point: *const u64, n_point: u64, out: *mut u64) -> i32;
    fn zk_cmle_to_bytes(ctx: *mut zk_ctx, p: *const zk_cmle, out_bytes: *mut u8) -> i32;
    fn zk_cmle_fixed_mask(p: *const zk_cmle, out: *mut u64) -> i32;
    fn zk_cmle_len(p: *const zk_cmle, out: *mut u64) -> i32;
    fn zk_cmle_partial_evaluate(ctx: *mut zk_ctx, p: *const zk_cmle, selectors: *const u8, selector_lens: *const u64,
                                values: *const u64, n_assign: u64, out: *mut *mut zk_cmle) -> i32;
    fn zk_cmle_relabel(ctx: *mut zk_ctx, p: *mut zk_cmle) -> i32;
    fn zk_cmle_scalar_multiply(ctx: *mut zk_ctx, p: *const zk_cmle, s: *const u64, out: *mut *mut zk_cmle) -> i32;
    fn zk_cmle_add(ctx: *mut zk_ctx, a: *const zk_cmle, b: *const zk_cmle, out: *mut *mut zk_cmle) -> i32;
    fn zk_cmle_mul(ctx: *mut zk_ctx, a: *const zk_cmle, b: *const zk_cmle, out: *mut *mut zk_cmle) -> i32;
    // batch inversion and running products (no reference item; include/zk_amd.h)
    fn zk_mle_alloc(ctx: *mut zk_ctx, n_vars: u64, out: *mut *mut zk_mle) -> i32;
    fn zk_mle_batch_inverse(ctx: *mut zk_ctx, t: *const zk_mle, shift: *const u64, out: *mut zk_mle, out_zeros: *mut u64) -> i32;
    fn zk_upoly_batch_inverse(ctx: *mut zk_ctx, v: *const zk_upoly, shift: *const u64, out: *mut *mut zk_upoly, out_zeros: *mut u64) -> i32;
    fn zk_mle_prefix_product(ctx: *mut zk_ctx, t: *const zk_mle, inclusive: i32, out: *mut zk_mle, out_total: *mut u64) -> i32;
    fn zk_batch_inverse_host(ctx: *mut zk_ctx, input: *const u64, n: u64, shift: *const u64, out: *mut u64, out_zeros: *mut u64) -> i32;
    // binary Merkle commitments over tables (no reference item; include/zk_amd.h)
    fn zk_merkle_commit(ctx: *mut zk_ctx, columns: *const *const zk_mle, n_columns: u32, out: *mut *mut zk_merkle) -> i32;
    fn zk_merkle_free(m: *mut zk_merkle) -> i32;
    fn zk_merkle_n_vars(m: *const zk_merkle, out: *mut u32) -> i32;
    fn zk_merkle_n_columns(m: *const zk_merkle, out: *mut u32) -> i32;
    fn zk_merkle_root(ctx: *mut zk_ctx, m: *const zk_merkle, out: *mut u8) -> i32;
    fn zk_merkle_level(ctx: *mut zk_ctx, m: *const zk_merkle, level: u32, out: *mut u8) -> i32;
    fn zk_merkle_open(ctx: *mut zk_ctx, m: *const zk_merkle, columns: *const *const zk_mle, n_columns: u32, indices: *const u64, n_queries: u64,
                      out_rows: *mut u64, out_paths: *mut u8) -> i32;
    fn zk_merkle_verify_host(field: i32, root: *const u8, n_vars: u32, n_columns: u32, index: u64, row: *const u64, path: *const u8,
                             out_ok: *mut i32) -> i32;
    // FRI low-degree proofs (no reference item; include/zk_amd.h)
    fn zk_fri_lde(ctx: *mut zk_ctx, p: *const zk_upoly, log_n: u32, shift: *const u64, out: *mut *mut zk_mle) -> i32;
    fn zk_fri_fold(ctx: *mut zk_ctx, input: *const zk_mle, log_arity: u32, shift: *const u64, beta: *const u64, out: *mut zk_mle) -> i32;
    fn zk_fri_proof_bytes(log_degree: u32, log_blowup: u32, log_arity: u32, log_final: u32, n_queries: u32, out: *mut u64) -> i32;
    fn zk_fri_prove(ctx: *mut zk_ctx, p: *const zk_upoly, log_degree: u32, log_blowup: u32, log_arity: u32, log_final: u32, n_queries: u32,
                    shift: *const u64, seed: *const u8, out_proof: *mut u8) -> i32;
    fn zk_fri_verify_host(field: i32, log_degree: u32, log_blowup: u32, log_arity: u32, log_final: u32, n_queries: u32, shift: *const u64,
                          seed: *const u8, proof: *const u8, proof_len: u64, out_ok: *mut i32) -> i32;
    // FRI polynomial commitment (no reference item; include/zk_amd.h)
    fn zk_deep_quotient(ctx: *mut zk_ctx, columns: *const *const zk_mle, n_columns: u32, shift: *const u64, z: *const u64, values: *const u64,
                        alpha: *const u64, out: *mut zk_mle) -> i32;
    fn zk_pcs_commit(ctx: *mut zk_ctx, polys: *const *const zk_upoly, k: u32, log_degree: u32, log_blowup: u32, log_arity: u32, shift: *const u64,
                     out: *mut *mut zk_pcs) -> i32;
    fn zk_pcs_free(h: *mut zk_pcs) -> i32;
    fn zk_pcs_n_polys(h: *const zk_pcs, out: *mut u32) -> i32;
    fn zk_pcs_root(ctx: *mut zk_ctx, h: *const zk_pcs, out: *mut u8) -> i32;
    fn zk_pcs_proof_bytes(k: u32, log_degree: u32, log_blowup: u32, log_arity: u32, log_final: u32, n_queries: u32, out: *mut u64) -> i32;
    fn zk_pcs_open(ctx: *mut zk_ctx, h: *const zk_pcs, z: *const u64, log_final: u32, n_queries: u32, seed: *const u8, out_values: *mut u64,
                   out_proof: *mut u8) -> i32;
    fn zk_pcs_verify_host(field: i32, k: u32, log_degree: u32, log_blowup: u32, log_arity: u32, log_final: u32, n_queries: u32, shift: *const u64,
                          seed: *const u8, root: *const u8, z: *const u64, values: *const u64, proof: *const u8, proof_len: u64,
                          out_ok: *mut i32) -> i32;
    // multilinear polynomial commitment (no reference item; include/zk_amd.h)
    fn zk_mlpcs_commit(ctx: *mut zk_ctx, table: *const zk_mle, log_blowup: u32, shift: *const u64, out: *mut *mut zk_mlpcs) -> i32;
    fn zk_mlpcs_free(h: *mut zk_mlpcs) -> i32;
    fn zk_mlpcs_n_vars(h: *const zk_mlpcs, out: *mut u32) -> i32;
    fn zk_mlpcs_root(ctx: *mut zk_ctx, h: *const zk_mlpcs, out: *mut u8) -> i32;
    fn zk_mlpcs_proof_bytes(n_vars: u32, log_blowup: u32, log_final: u32, n_queries: u32, out: *mut u64) -> i32;
    fn zk_mlpcs_open(ctx: *mut zk_ctx, h: *const zk_mlpcs, point: *const u64, n_point: u64, log_final: u32, n_queries: u32, seed: *const u8,
                     out_value: *mut u64, out_proof: *mut u8) -> i32;
    fn zk_mlpcs_verify_host(field: i32, n_vars: u32, log_blowup: u32, log_final: u32, n_queries: u32, shift: *const u64, seed: *const u8,
                            root: *const u8, point: *const u64, value: *const u64, proof: *const u8, proof_len: u64, out_ok: *mut i32) -> i32;
    fn zk_mle_eq_sums(ctx: *mut zk_ctx, t: *const zk_mle, tail: *const u64, out: *mut u64) -> i32;
    fn zk_mlbatch_commit(ctx: *mut zk_ctx, tables: *const *const zk_mle, k: u32, log_blowup: u32, shift: *const u64, out: *mut *mut zk_mlbatch) -> i32;
    fn zk_mlbatch_free(h: *mut zk_mlbatch) -> i32;
    fn zk_mlbatch_n_vars(h: *const zk_mlbatch, out: *mut u32) -> i32;
    fn zk_mlbatch_n_tables(h: *const zk_mlbatch, out: *mut u32) -> i32;
    fn zk_mlbatch_root(ctx: *mut zk_ctx, h: *const zk_mlbatch, out: *mut u8) -> i32;
    fn zk_mlbatch_proof_bytes(n_vars: u32, k: u32, n_points: u32, log_blowup: u32, log_final: u32, n_queries: u32, out: *mut u64) -> i32;
    fn zk_mlbatch_open(ctx: *mut zk_ctx, h: *const zk_mlbatch, points: *const u64, n_points: u32, log_final: u32, n_queries: u32, seed: *const u8,
                       out_values: *mut u64, out_proof: *mut u8) -> i32;
    fn zk_mlbatch_verify_host(field: i32, n_vars: u32, k: u32, n_points: u32, log_blowup: u32, log_final: u32, n_queries: u32, shift: *const u64,
                              seed: *const u8, root: *const u8, points: *const u64, values: *const u64, proof: *const u8, proof_len: u64,
                              out_ok: *mut i32) -> i32;
    fn zk_mle_lincomb(ctx: *mut zk_ctx, tables: *const *const zk_mle, k: u32, coeffs: *const u64, out: *mut zk_mle) -> i32;
    fn zk_mle_eq_sums_many(ctx: *mut zk_ctx, t: *const zk_mle, tails: *const u64, n_points: u32, out: *mut u64) -> i32;
    fn zk_mle_product_tree(ctx: *mut zk_ctx, t: *const zk_mle, shift: *const u64, out: *mut *mut zk_mle) -> i32;
    fn zk_gprod_proof_bytes(n_vars: u32, out: *mut u64) -> i32;
    fn zk_gprod_prove(ctx: *mut zk_ctx, t: *const zk_mle, shift: *const u64, seed: *const u8, out_product: *mut u64, out_proof: *mut u8,
                      out_point: *mut u64, out_claim: *mut u64) -> i32;
    fn zk_gprod_verify_host(field: i32, n_vars: u32, shift: *const u64, seed: *const u8, product: *const u64, proof: *const u8, proof_len: u64,
                            out_point: *mut u64, out_claim: *mut u64, out_ok: *mut i32) -> i32;
    fn zk_mle_fraction_tree(ctx: *mut zk_ctx, p: *const zk_mle, q: *const zk_mle, shift: *const u64, out_p: *mut *mut zk_mle, out_q: *mut *mut zk_mle) -> i32;
    fn zk_fsum_proof_bytes(n_vars: u32, out: *mut u64) -> i32;
    fn zk_fsum_prove(ctx: *mut zk_ctx, p: *const zk_mle, q: *const zk_mle, shift: *const u64, seed: *const u8, out_sum: *mut u64, out_proof: *mut u8,
                     out_point: *mut u64, out_claims: *mut u64) -> i32;
    fn zk_fsum_verify_host(field: i32, n_vars: u32, has_p: i32, shift: *const u64, seed: *const u8, sum: *const u64, proof: *const u8, proof_len: u64,
                           out_point: *mut u64, out_claims: *mut u64, out_ok: *mut i32) -> i32;
    fn zk_lookup_multiplicities(ctx: *mut zk_ctx, table: *const zk_mle, witness: *const zk_mle, out_m: *mut *mut zk_mle, out_missing: *mut u64,
                                out_first_missing: *mut u64, out_duplicates: *mut u64) -> i32;
    fn zk_gate_create(field: i32, k: u32, n_terms: u32, coeffs: *const u64, term_len: *const u32, factors: *const u32, out: *mut *mut zk_gate) -> i32;
    fn zk_gate_free(gate: *mut zk_gate) -> i32;
    fn zk_gate_degree(gate: *const zk_gate, out: *mut u32) -> i32;
    fn zk_gate_n_columns(gate: *const zk_gate, out: *mut u32) -> i32;
    fn zk_zerocheck_proof_bytes(gate: *const zk_gate, n_vars: u32, out: *mut u64) -> i32;
    fn zk_zerocheck_prove(ctx: *mut zk_ctx, tables: *const *const zk_mle, gate: *const zk_gate, seed: *const u8, out_proof: *mut u8,
                          out_point: *mut u64, out_claims: *mut u64) -> i32;
    fn zk_zerocheck_verify_host(gate: *const zk_gate, n_vars: u32, seed: *const u8, proof: *const u8, proof_len: u64, out_point: *mut u64,
                                out_claims: *mut u64, out_ok: *mut i32) -> i32;
    fn zk_mle_gate_sums(ctx: *mut zk_ctx, tables: *const *const zk_mle, gate: *const zk_gate, tail: *const u64, out: *mut u64) -> i32;
    fn zk_perm_proof_bytes(n_vars: u32, k: u32, out: *mut u64) -> i32;
    fn zk_mle_perm_fingerprint(ctx: *mut zk_ctx, w: *const *const zk_mle, sigma: *const *const zk_mle, k: u32, beta: *const u64, gamma: *const u64,
                               out: *mut *mut zk_mle) -> i32;
    fn zk_perm_prove(ctx: *mut zk_ctx, w: *const *const zk_mle, sigma: *const *const zk_mle, k: u32, beta: *const u64, gamma: *const u64,
                     seed: *const u8, out_proof: *mut u8, out_point: *mut u64, out_claims: *mut u64) -> i32;
    fn zk_perm_verify_host(field: i32, n_vars: u32, k: u32, beta: *const u64, gamma: *const u64, seed: *const u8, proof: *const u8, proof_len: u64,
                           out_point: *mut u64, out_claims: *mut u64, out_ok: *mut i32) -> i32;
    fn zk_product_check(factors: *const *const zk_mle, k: u64) -> i32;
    fn zk_prod_reduce(ctx: *mut zk_ctx, factors: *const *const zk_mle, k: u64, out: *mut *mut zk_mle) -> i32;
    fn zk_product_evaluate(ctx: *mut zk_ctx, factors: *const *const zk_mle, k: u64, point: *const u64, n_point: u64,
                           out: *mut u64) -> i32;
    fn zk_transcript_new(out: *mut *mut zk_transcript) -> i32;
    fn zk_transcript_free(t: *mut zk_transcript) -> i32;
    fn zk_transcript_append(t: *mut zk_transcript, data: *const u8, len: usize) -> i32;
    fn zk_transcript_sample_field_element(t: *mut zk_transcript, field: i32, out: *mut u64) -> i32;
    fn zk_transcript_sample_n_field_elements(t: *mut zk_transcript, field: i32, n: u64, out: *mut u64) -> i32;
    fn zk_sumcheck_prove(ctx: *mut zk_ctx, factors: *const *mut zk_mle, k: u64, max_var_degree: u32, sum: *const u64,
                         absorb_table: i32, consume: i32, out_round_polys: *mut u64, out_challenges: *mut u64) -> i32;
    fn zk_sumcheck_prove_batch(ctx: *mut zk_ctx, n_proofs: u64, factors: *const *mut zk_mle, k: u64, max_var_degree: u32, sums: *const u64,
                               consume: i32, out_round_polys: *mut u64, out_challenges: *mut u64) -> i32;
    fn zk_sumcheck_verify_partial(field: i32, n_rounds: u64, max_var_degree: u32, sum: *const u64, round_polys: *const u64,
                                  out_subclaim_sum: *mut u64, out_challenges: *mut u64) -> i32;
    fn zk_sumcheck_verify(ctx: *mut zk_ctx, factors: *const *const zk_mle, k: u64, n_round_polys: u64, max_var_degree: u32,
                          sum: *const u64, round_polys: *const u64, out_ok: *mut i32) -> i32;
    fn zk_sumcheck_verify_partial_lengths(field: i32, n_rounds: u64, evals_per_round: *const u32, sum: *const u64,
                                          round_polys: *const u64, out_subclaim_sum: *mut u64, out_challenges: *mut u64) -> i32;
    fn zk_sumcheck_verify_lengths(ctx: *mut zk_ctx, factors: *const *const zk_mle, k: u64, n_round_polys: u64,
                                  evals_per_round: *const u32, sum: *const u64, round_polys: *const u64, out_ok: *mut i32) -> i32;
    fn zk_fft_host(ctx: *mut zk_ctx, input: *const u64, n: u64, out: *mut u64) -> i32;
    fn zk_ifft_host(ctx: *mut zk_ctx, input: *const u64, n: u64, out: *mut u64) -> i32;
    fn zk_fft_internal_host(ctx: *mut zk_ctx, input: *const u64, n: u64, omega: *const u64, out: *mut u64) -> i32;
    // GKR-shaped driver (no reference crate; include/zk_amd.h "sum of products + GKR-shaped driver")
    fn zk_sumcheck_prove_terms(ctx: *mut zk_ctx, factors: *const *mut zk_mle, term_k: *const u64, n_terms: u64,
                               max_var_degree: u32, sum: *const u64, consume: i32, out_round_polys: *mut u64,
                               out_challenges: *mut u64, out_final: *mut u64) -> i32;
    fn zk_circuit_create(ctx: *mut zk_ctx, out: *mut *mut zk_circuit) -> i32;
    fn zk_circuit_add_layer(c: *mut zk_circuit, log_out: u64, log_in: u64, op: *const u8, left: *const u32,
                            right: *const u32) -> i32;
    fn zk_circuit_free(c: *mut zk_circuit) -> i32;
    fn zk_circuit_proof_elems(c: *const zk_circuit, out: *mut u64) -> i32;
    fn zk_gkr_prove(c: *const zk_circuit, input: *const zk_mle, seed: *const u8, out_outputs: *mut *mut zk_mle,
                    out_proof: *mut u64) -> i32;
    fn zk_gkr_verify(c: *const zk_circuit, input: *const zk_mle, outputs: *const zk_mle, seed: *const u8,
                     proof: *const u64) -> i32;
}

/// Maps an arkworks field onto libzk_amd's `zk_field` enum (only 4-limb Montgomery fields qualify).
pub trait GpuField: PrimeField {
    const ZK_FIELD: i32;
}
impl GpuField for ark_bn254::Fr { const ZK_FIELD: i32 = 0; }
impl GpuField for ark_bls12_381::Fr { const ZK_FIELD: i32 = 1; }
impl GpuField for ark_bls12_377::Fr { const ZK_FIELD: i32 = 2; }
// `limbs()` below hands `&[F]` to C as `*const u64`: that is only sound while an element IS four u64 limbs.  Checked at
// compile time for every field the library is bound to (polynomial/src/multilinear/evaluation_form.rs:7-10 stores Vec<F>).
const _: () = assert!(std::mem::size_of::<ark_bn254::Fr>() == 32 && std::mem::align_of::<ark_bn254::Fr>() == 8);
const _: () = assert!(std::mem::size_of::<ark_bls12_381::Fr>() == 32 && std::mem::align_of::<ark_bls12_381::Fr>() == 8);
const _: () = assert!(std::mem::size_of::<ark_bls12_377::Fr>() == 32 && std::mem::align_of::<ark_bls12_377::Fr>() == 8);

fn err(status: i32) -> &'static str {
    // zk_strerror returns pointers to static strings that reproduce the reference's own messages
    unsafe { std::ffi::CStr::from_ptr(zk_strerror(status)).to_str().unwrap_or("zk_amd error") }
}

/// One `zk_ctx` (device + stream + scratch + block pool); destroyed with its last `Rc`.
struct Ctx { raw: *mut zk_ctx }
impl Drop for Ctx {
    fn drop(&mut self) { unsafe { zk_ctx_destroy(self.raw); } }
}
thread_local! {
    static CTXS: RefCell<[Option<Rc<Ctx>>; 3]> = const { RefCell::new([None, None, None]) };
}
/// The calling thread's context for field `F`: created on first use, then shared (tables built independently by `new`
/// therefore always belong to one context and can be combined in a `ProductPoly`).
fn ctx<F: GpuField>() -> Result<Rc<Ctx>, &'static str> {
    CTXS.with(|cell| {
        let mut slots = cell.borrow_mut();
        let slot = &mut slots[F::ZK_FIELD as usize];
        if let Some(c) = slot { return Ok(Rc::clone(c)); }
        // a libzk_amd.so of another ABI revision must not be driven through these declarations
        if unsafe { zk_abi_version() } != ZK_AMD_ABI_VERSION { return Err("zk_amd: libzk_amd.so ABI version mismatch"); }
        let device = std::env::var("ZK_AMD_DEVICE").ok().and_then(|s| s.parse::<i32>().ok()).unwrap_or(0);
        let mut raw: *mut zk_ctx = std::ptr::null_mut();
        let rc = unsafe { zk_ctx_create(F::ZK_FIELD, device, &mut raw) };
        if rc != 0 { return Err(err(rc)); }
        let c = Rc::new(Ctx { raw });
        *slot = Some(Rc::clone(&c));
        Ok(c)
    })
}
/// polynomial/src/multilinear/pairing_index.rs:24-26 — a bit sequence of n ones (`mask(1) -> 1`, `mask(3) -> 0b111`); public in the
/// reference, so part of the surface a caller may use.  Overflows (a panic in debug builds) at n >= usize::BITS like the original.
pub const fn mask(n: u8) -> usize {
    (1 << n) - 1
}

/// `&[F]` as the limb array the C ABI expects (ark-ff stores exactly this).
fn limbs<F: GpuField>(v: &[F]) -> *const u64 { v.as_ptr() as *const u64 }
fn limbs_mut<F: GpuField>(v: &mut [F]) -> *mut u64 { v.as_mut_ptr() as *mut u64 }

/// polynomial/src/multilinear/pairing_index.rs:2-9 — the (left, right) index pairs of one hypercube direction.
/// Host index arithmetic only (the kernels compute the same indices inline); panics on underflow like the reference.
pub fn index_pair(n_vars: u8, index: u8) -> impl Iterator<Item = (usize, usize)> {
    let pos = n_vars - 1 - index;
    (0..1usize << (n_vars - 1)).map(move |j| {
        let left = ((j >> pos) << (pos + 1)) | (j & mask(pos));
        (left, left | (1usize << pos))
    })
}

/// polynomial::multilinear::evaluation_form::MultiLinearPolynomial (evaluation_form.rs:7-10), table resident in HBM.
pub struct MultiLinearPolynomial<F: GpuField> {
    ctx: Rc<Ctx>,
    h: *mut zk_mle,
    n_vars: usize,
    host: OnceCell<Vec<F>>, // lazily downloaded mirror backing `evaluation_slice`; tables are immutable once built
}

impl<F: GpuField> Drop for MultiLinearPolynomial<F> {
    fn drop(&mut self) { unsafe { zk_mle_free(self.ctx.raw, self.h); } }
}
/// #[derive(Clone)] evaluation_form.rs:4 — a device-to-device copy
impl<F: GpuField> Clone for MultiLinearPolynomial<F> {
    fn clone(&self) -> Self {
        let mut h: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_mle_clone(self.ctx.raw, self.h, &mut h) };
        assert!(rc == 0, "{}", err(rc));
        Self::from_handle(Rc::clone(&self.ctx), h)
    }
}
/// #[derive(PartialEq)] evaluation_form.rs:4 — n_vars and all evaluations, compared on the device
impl<F: GpuField> PartialEq for MultiLinearPolynomial<F> {
    fn eq(&self, other: &Self) -> bool {
        if self.n_vars != other.n_vars { return false; }
        if !Rc::ptr_eq(&self.ctx, &other.ctx) { return self.evaluation_slice() == other.evaluation_slice(); }
        let mut eq = 0i32;
        let rc = unsafe { zk_mle_equal(self.ctx.raw, self.h, other.h, &mut eq) };
        assert!(rc == 0, "{}", err(rc));
        eq != 0
    }
}
/// #[derive(Debug)] evaluation_form.rs:4
impl<F: GpuField> fmt::Debug for MultiLinearPolynomial<F> {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        f.debug_struct("MultiLinearPolynomial").field("n_vars", &self.n_vars).field("evaluations", &self.evaluation_slice()).finish()
    }
}
impl<F: GpuField> MultiLinearPolynomial<F> {
    fn from_handle(ctx: Rc<Ctx>, h: *mut zk_mle) -> Self {
        let mut n = 0u64;
        unsafe { zk_mle_n_vars(h, &mut n); }
        Self { ctx, h, n_vars: n as usize, host: OnceCell::new() }
    }
    /// evaluation_form.rs:15-27
    pub fn new(n_vars: usize, evaluations: Vec<F>) -> Result<Self, &'static str> {
        let c = ctx::<F>()?;
        let mut h: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_mle_upload(c.raw, n_vars as u64, limbs(&evaluations), evaluations.len() as u64, &mut h) };
        if rc != 0 { return Err(err(rc)); } // "evaluation vec len should equal 2^n_vars"
        Ok(Self { ctx: c, h, n_vars, host: OnceCell::from(evaluations) }) // the caller's Vec IS the host mirror
    }
    /// Shard `rank` of `world` of the table `new(n_vars, evaluations)` would make: {idx : idx mod world == rank}, local index
    /// idx / world (the layout of the sharded prover and NTT).  Only the shard goes to the device.
    pub fn new_shard(n_vars: usize, evaluations: &[F], world: u32, rank: u32) -> Result<Self, &'static str> {
        let c = ctx::<F>()?;
        let mut h: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_mle_upload_shard(c.raw, n_vars as u64, limbs(evaluations), evaluations.len() as u64, world, rank, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self::from_handle(c, h))
    }
    /// All `world` shards by index mod world, in rank order, in one pass on the device; `self` is unchanged.
    pub fn split(&self, world: u32) -> Result<Vec<Self>, &'static str> {
        let mut hs: Vec<*mut zk_mle> = vec![std::ptr::null_mut(); world.max(1) as usize];
        let rc = unsafe { zk_mle_split(self.ctx.raw, self.h, world, hs.as_mut_ptr()) };
        if rc != 0 { return Err(err(rc)); }
        Ok(hs.into_iter().take(world as usize).map(|h| Self::from_handle(Rc::clone(&self.ctx), h)).collect())
    }
    /// Inverse of `split`: equal-size shards in rank order -> the natural-order table.
    pub fn interleave(shards: &[Self]) -> Result<Self, &'static str> {
        let first = shards.first().ok_or("bad argument")?;
        let hs: Vec<*const zk_mle> = shards.iter().map(|s| s.h as *const zk_mle).collect();
        let mut h: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_mle_interleave(first.ctx.raw, hs.as_ptr(), hs.len() as u32, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self::from_handle(Rc::clone(&first.ctx), h))
    }
    /// evaluation_form.rs:30
    pub fn n_vars(&self) -> usize { self.n_vars }
    /// evaluation_form.rs:40-80
    pub fn partial_evaluate(&self, initial_var: usize, assignments: &[F]) -> Result<Self, &'static str> {
        let mut h: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_mle_partial_evaluate(self.ctx.raw, self.h, initial_var as u64, limbs(assignments),
                                                  assignments.len() as u64, &mut h) };
        if rc == ZK_ERR_PANIC_INDEX { panic!("{}", err(rc)); } // the reference panics here (u8 / usize underflow, :55,:75)
        if rc != 0 { return Err(err(rc)); }
        Ok(Self::from_handle(Rc::clone(&self.ctx), h))
    }
    /// evaluation_form.rs:83-89
    pub fn evaluate(&self, assignments: &[F]) -> Result<F, &'static str> {
        let mut out = [F::zero()];
        let rc = unsafe { zk_mle_evaluate(self.ctx.raw, self.h, limbs(assignments), assignments.len() as u64, limbs_mut(&mut out)) };
        if rc != 0 { return Err(err(rc)); } // "evaluate must assign to all variables"
        Ok(out[0])
    }
    /// evaluation_form.rs:92-94 — a borrowed slice, like the reference; the first call on a table that was produced on the
    /// device downloads it once (2^n_vars * 32 bytes over PCIe): keep tables on the device where speed matters.
    pub fn evaluation_slice(&self) -> &[F] {
        self.host.get_or_init(|| {
            let mut v = vec![F::zero(); 1usize << self.n_vars];
            let rc = unsafe { zk_mle_download(self.ctx.raw, self.h, limbs_mut(&mut v)) };
            assert!(rc == 0, "{}", err(rc));
            v
        })
    }
    /// evaluation_form.rs:97-103
    pub fn to_bytes(&self) -> Vec<u8> {
        let mut b = vec![0u8; 32usize << self.n_vars];
        let rc = unsafe { zk_mle_to_bytes(self.ctx.raw, self.h, b.as_mut_ptr()) };
        assert!(rc == 0, "{}", err(rc));
        b
    }
    fn alloc_like(&self) -> Result<Self, &'static str> {
        let mut h: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_mle_alloc(self.ctx.raw, self.n_vars as u64, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self::from_handle(Rc::clone(&self.ctx), h))
    }
    /// Batch inversion (the reference has none; include/zk_amd.h, zk_mle_batch_inverse): a new table of `1 / (t[i] + shift)`,
    /// zero where the denominator is zero, and the number of such zeros (ark-ff's batch_inversion rule: skipped, not an error).
    pub fn batch_inverse(&self, shift: Option<&F>) -> Result<(Self, u64), &'static str> {
        let out = self.alloc_like()?;
        let mut zeros = 0u64;
        let sp = shift.map_or(std::ptr::null(), |s| limbs(std::slice::from_ref(s)));
        let rc = unsafe { zk_mle_batch_inverse(self.ctx.raw, self.h, sp, out.h, &mut zeros) };
        if rc != 0 { return Err(err(rc)); }
        Ok((out, zeros))
    }
    /// Running product (include/zk_amd.h, zk_mle_prefix_product): exclusive `out[0] = 1, out[i] = t[0] ... t[i-1]`, or inclusive
    /// `out[i] = t[0] ... t[i]`, and the product of all elements.  A zero propagates.
    pub fn prefix_product(&self, inclusive: bool) -> Result<(Self, F), &'static str> {
        let out = self.alloc_like()?;
        let mut total = [F::zero()];
        let rc = unsafe { zk_mle_prefix_product(self.ctx.raw, self.h, inclusive as i32, out.h, limbs_mut(&mut total)) };
        if rc != 0 { return Err(err(rc)); }
        Ok((out, total[0]))
    }
}

/// polynomial::univariate_poly::UnivariatePolynomial (univariate_poly.rs:7-12): coefficients lowest degree first, resident in
/// HBM.  `new`, `evaluate` and `Mul` cannot fail in the reference, so a library error (no device; a product longer than the
/// supported transform, include/zk_amd.h zk_upoly_mul) panics with the library's message.
pub struct UnivariatePolynomial<F: GpuField> {
    ctx: Rc<Ctx>,
    h: *mut zk_upoly,
    len: usize,
    host: OnceCell<Vec<F>>, // lazily downloaded mirror backing `coefficients`; immutable once built
}
impl<F: GpuField> Drop for UnivariatePolynomial<F> {
    fn drop(&mut self) { unsafe { zk_upoly_free(self.ctx.raw, self.h); } }
}
/// #[derive(Clone)] univariate_poly.rs:7
impl<F: GpuField> Clone for UnivariatePolynomial<F> {
    fn clone(&self) -> Self { Self::new(self.coefficients().to_vec()) }
}
/// #[derive(PartialEq)] univariate_poly.rs:7 — the coefficient vectors (trailing zeros count)
impl<F: GpuField> PartialEq for UnivariatePolynomial<F> {
    fn eq(&self, other: &Self) -> bool { self.coefficients() == other.coefficients() }
}
/// #[derive(Debug)] univariate_poly.rs:7
impl<F: GpuField> fmt::Debug for UnivariatePolynomial<F> {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        f.debug_struct("UnivariatePolynomial").field("coefficients", &self.coefficients()).finish()
    }
}
impl<F: GpuField> UnivariatePolynomial<F> {
    fn from_handle(ctx: Rc<Ctx>, h: *mut zk_upoly) -> Self {
        let mut n = 0u64;
        unsafe { zk_upoly_len(h, &mut n); }
        Self { ctx, h, len: n as usize, host: OnceCell::new() }
    }
    /// univariate_poly.rs:16-19
    pub fn new(coefficients: Vec<F>) -> Self {
        let c = ctx::<F>().unwrap_or_else(|e| panic!("{}", e));
        let mut h: *mut zk_upoly = std::ptr::null_mut();
        let rc = unsafe { zk_upoly_upload(c.raw, limbs(&coefficients), coefficients.len() as u64, &mut h) };
        assert!(rc == 0, "{}", err(rc));
        let len = coefficients.len();
        Self { ctx: c, h, len, host: OnceCell::from(coefficients) } // the caller's Vec IS the host mirror
    }
    /// univariate_poly.rs:21-23 — the first call on a product computed on the device downloads it once
    pub fn coefficients(&self) -> &[F] {
        self.host.get_or_init(|| {
            let mut v = vec![F::zero(); self.len];
            let rc = unsafe { zk_upoly_download(self.ctx.raw, self.h, limbs_mut(&mut v)) };
            assert!(rc == 0, "{}", err(rc));
            v
        })
    }
    /// univariate_poly.rs:29-40
    pub fn evaluate(&self, x: &F) -> F {
        let mut out = [F::zero()];
        let rc = unsafe { zk_upoly_evaluate(self.ctx.raw, self.h, limbs(std::slice::from_ref(x)), limbs_mut(&mut out)) };
        assert!(rc == 0, "{}", err(rc));
        out[0]
    }
    /// univariate_poly.rs:43-49 — xs = 0 .. n-1; exactly n coefficients
    pub fn interpolate(ys: Vec<F>) -> Self {
        let y = Self::new(ys);
        let mut h: *mut zk_upoly = std::ptr::null_mut();
        let rc = unsafe { zk_upoly_interpolate(y.ctx.raw, y.h, &mut h) };
        assert!(rc == 0, "{}", err(rc));
        Self::from_handle(Rc::clone(&y.ctx), h)
    }
    /// univariate_poly.rs:54-80 — panics with the library's message where the reference panics (a repeated x, :68)
    pub fn interpolate_xy(xs: Vec<F>, ys: Vec<F>) -> Self {
        let (x, y) = (Self::new(xs), Self::new(ys));
        let mut h: *mut zk_upoly = std::ptr::null_mut();
        let rc = unsafe { zk_upoly_interpolate_xy(x.ctx.raw, x.h, y.h, &mut h) };
        assert!(rc == 0, "{}", err(rc));
        Self::from_handle(Rc::clone(&x.ctx), h)
    }
    /// univariate_poly.rs:29-40 at every point of `xs` (a polynomial used as a vector of points): the values stay on the device,
    /// no host wait.  Err where the shape is past the library's length rule (include/zk_amd.h, zk_upoly_evaluate_many).
    pub fn evaluate_many(&self, xs: &Self) -> Result<Self, &'static str> {
        let mut h: *mut zk_upoly = std::ptr::null_mut();
        let rc = unsafe { zk_upoly_evaluate_many(self.ctx.raw, self.h, xs.h, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self::from_handle(Rc::clone(&self.ctx), h))
    }
    /// Division with remainder (the reference has none; include/zk_amd.h, zk_upoly_divrem): `(q, r)` with `self = q * b + r`,
    /// `len(q) = len - len(b) + 1`, `len(r) = len(b) - 1`, nothing trimmed.  Err for an empty `b`, a zero last coefficient of `b`
    /// (it is inverted) and shapes past the library's length rule.
    pub fn divrem(&self, b: &Self) -> Result<(Self, Self), &'static str> {
        let mut q: *mut zk_upoly = std::ptr::null_mut();
        let mut r: *mut zk_upoly = std::ptr::null_mut();
        let rc = unsafe { zk_upoly_divrem(self.ctx.raw, self.h, b.h, &mut q, &mut r) };
        if rc != 0 { return Err(err(rc)); }
        Ok((Self::from_handle(Rc::clone(&self.ctx), q), Self::from_handle(Rc::clone(&self.ctx), r)))
    }
    /// Batch inversion of the coefficient vector (include/zk_amd.h, zk_upoly_batch_inverse): `1 / (v[i] + shift)`, zero where the
    /// denominator is zero, and the number of such zeros.  Any length, 0 included.
    pub fn batch_inverse(&self, shift: Option<&F>) -> Result<(Self, u64), &'static str> {
        let mut h: *mut zk_upoly = std::ptr::null_mut();
        let mut zeros = 0u64;
        let sp = shift.map_or(std::ptr::null(), |s| limbs(std::slice::from_ref(s)));
        let rc = unsafe { zk_upoly_batch_inverse(self.ctx.raw, self.h, sp, &mut h, &mut zeros) };
        if rc != 0 { return Err(err(rc)); }
        Ok((Self::from_handle(Rc::clone(&self.ctx), h), zeros))
    }
    /// The `k` coefficients of `1 / self mod z^k`; Err for `self[0] = 0`, an empty `self` and `k` past the length rule.
    pub fn inverse_series(&self, k: u64) -> Result<Self, &'static str> {
        let mut h: *mut zk_upoly = std::ptr::null_mut();
        let rc = unsafe { zk_upoly_inverse_series(self.ctx.raw, self.h, k, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self::from_handle(Rc::clone(&self.ctx), h))
    }
}
/// Value-semantics batch inversion (include/zk_amd.h, zk_batch_inverse_host): `1 / (values[i] + shift)` with zeros left zero,
/// and the number of zeros.
pub fn batch_inverse<F: GpuField>(values: &[F], shift: Option<&F>) -> Result<(Vec<F>, u64), &'static str> {
    let c = ctx::<F>()?;
    let mut out = vec![F::zero(); values.len()];
    let mut zeros = 0u64;
    let sp = shift.map_or(std::ptr::null(), |s| limbs(std::slice::from_ref(s)));
    let rc = unsafe { zk_batch_inverse_host(c.raw, limbs(values), values.len() as u64, sp, limbs_mut(&mut out), &mut zeros) };
    if rc != 0 { return Err(err(rc)); }
    Ok((out, zeros))
}
/// Binary Keccak-256 Merkle commitment over `k` tables of `2^n` elements, every level resident in HBM (include/zk_amd.h, zk_merkle;
/// the reference has none).  Leaf `i` hashes the 32-byte big-endian canonical images of row `i` of all columns.
pub struct MerkleTree<F: GpuField> { ctx: Rc<Ctx>, h: *mut zk_merkle, _f: PhantomData<F> }
impl<F: GpuField> Drop for MerkleTree<F> { fn drop(&mut self) { unsafe { zk_merkle_free(self.h); } } }
impl<F: GpuField> MerkleTree<F> {
    /// Stream-ordered, no host wait; the tree does not refer to the columns afterwards.
    pub fn commit(columns: &[&MultiLinearPolynomial<F>]) -> Result<Self, &'static str> {
        let c = ctx::<F>()?;
        let hs: Vec<*const zk_mle> = columns.iter().map(|t| t.h as *const zk_mle).collect();
        let mut h: *mut zk_merkle = std::ptr::null_mut();
        let rc = unsafe { zk_merkle_commit(c.raw, hs.as_ptr(), hs.len() as u32, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self { ctx: c, h, _f: PhantomData })
    }
    pub fn n_vars(&self) -> usize {
        let mut n = 0u32;
        unsafe { zk_merkle_n_vars(self.h, &mut n) };
        n as usize
    }
    pub fn n_columns(&self) -> usize {
        let mut k = 0u32;
        unsafe { zk_merkle_n_columns(self.h, &mut k) };
        k as usize
    }
    pub fn root(&self) -> Result<[u8; 32], &'static str> {
        let mut d = [0u8; 32];
        let rc = unsafe { zk_merkle_root(self.ctx.raw, self.h, d.as_mut_ptr()) };
        if rc != 0 { return Err(err(rc)); }
        Ok(d)
    }
    /// The `2^(n - level)` digests of one level, 32 bytes each.
    pub fn level(&self, level: u32) -> Result<Vec<u8>, &'static str> {
        if level as usize > self.n_vars() { return Err(err(ZK_ERR_BAD_ARG)); }
        let mut out = vec![0u8; 32usize << (self.n_vars() - level as usize)];
        let rc = unsafe { zk_merkle_level(self.ctx.raw, self.h, level, out.as_mut_ptr()) };
        if rc != 0 { return Err(err(rc)); }
        Ok(out)
    }
    /// The openings of the rows `indices`: (rows, paths) with `indices.len() * k` elements (empty without columns) and
    /// `indices.len() * n * 32` path bytes, the siblings bottom up.
    pub fn open(&self, indices: &[u64], columns: Option<&[&MultiLinearPolynomial<F>]>) -> Result<(Vec<F>, Vec<u8>), &'static str> {
        let hs: Vec<*const zk_mle> = columns.map_or(Vec::new(), |cs| cs.iter().map(|t| t.h as *const zk_mle).collect());
        let mut rows = vec![F::zero(); if columns.is_some() { indices.len() * self.n_columns() } else { 0 }];
        let mut paths = vec![0u8; indices.len() * self.n_vars() * 32];
        let cp = if columns.is_some() { hs.as_ptr() } else { std::ptr::null() };
        let rc = unsafe {
            zk_merkle_open(self.ctx.raw, self.h, cp, hs.len() as u32, indices.as_ptr(), indices.len() as u64, limbs_mut(&mut rows), paths.as_mut_ptr())
        };
        if rc != 0 { return Err(err(rc)); }
        Ok((rows, paths))
    }
}
/// Host only (include/zk_amd.h, zk_merkle_verify_host): does `path` (`n_vars` digests, bottom up) lead from the leaf of `row` at
/// `index` to `root`?
pub fn merkle_verify<F: GpuField>(root: &[u8; 32], n_vars: u32, index: u64, row: &[F], path: &[u8]) -> Result<bool, &'static str> {
    if path.len() != 32 * n_vars as usize { return Err(err(ZK_ERR_BAD_ARG)); }
    let mut ok = 0i32;
    let rc = unsafe { zk_merkle_verify_host(F::ZK_FIELD, root.as_ptr(), n_vars, row.len() as u32, index, limbs(row), path.as_ptr(), &mut ok) };
    if rc != 0 { return Err(err(rc)); }
    Ok(ok != 0)
}
/// FRI low-degree proofs (include/zk_amd.h, zk_fri_*; the reference has none): the parameters of one proof.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct FriParams { pub log_degree: u32, pub log_blowup: u32, pub log_arity: u32, pub log_final: u32, pub n_queries: u32 }
/// The evaluations of `p` (at most `2^log_n` coefficients) over `shift * <root_of_unity(2^log_n)>`, natural order.
pub fn fri_lde<F: GpuField>(p: &UnivariatePolynomial<F>, log_n: u32, shift: &F) -> Result<MultiLinearPolynomial<F>, &'static str> {
    let mut h: *mut zk_mle = std::ptr::null_mut();
    let rc = unsafe { zk_fri_lde(p.ctx.raw, p.h, log_n, limbs(std::slice::from_ref(shift)), &mut h) };
    if rc != 0 { return Err(err(rc)); }
    Ok(MultiLinearPolynomial::from_handle(Rc::clone(&p.ctx), h))
}
/// `layer` over the coset of `shift`, folded by `2^log_arity` at `beta`: a new table of `n_vars - log_arity` variables.
pub fn fri_fold<F: GpuField>(layer: &MultiLinearPolynomial<F>, log_arity: u32, shift: &F, beta: &F) -> Result<MultiLinearPolynomial<F>, &'static str> {
    if (layer.n_vars as u32) < log_arity { return Err(err(-1)); }
    let mut h: *mut zk_mle = std::ptr::null_mut();
    let rc = unsafe { zk_mle_alloc(layer.ctx.raw, (layer.n_vars as u32 - log_arity) as u64, &mut h) };
    if rc != 0 { return Err(err(rc)); }
    let out = MultiLinearPolynomial::from_handle(Rc::clone(&layer.ctx), h);
    let rc = unsafe { zk_fri_fold(layer.ctx.raw, layer.h, log_arity, limbs(std::slice::from_ref(shift)), limbs(std::slice::from_ref(beta)), out.h) };
    if rc != 0 { return Err(err(rc)); }
    Ok(out)
}
pub fn fri_proof_bytes(fp: &FriParams) -> Result<u64, &'static str> {
    let mut n = 0u64;
    let rc = unsafe { zk_fri_proof_bytes(fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries, &mut n) };
    if rc != 0 { return Err(err(rc)); }
    Ok(n)
}
/// The proof bytes: the roots, the final coefficients, and per query and round the opened row and its path.
pub fn fri_prove<F: GpuField>(p: &UnivariatePolynomial<F>, fp: &FriParams, shift: &F, seed: &[u8; 32]) -> Result<Vec<u8>, &'static str> {
    let mut proof = vec![0u8; fri_proof_bytes(fp)? as usize];
    let rc = unsafe {
        zk_fri_prove(p.ctx.raw, p.h, fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries, limbs(std::slice::from_ref(shift)),
                     seed.as_ptr(), proof.as_mut_ptr())
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(proof)
}
/// Host only (zk_fri_verify_host): needs no device.
pub fn fri_verify<F: GpuField>(proof: &[u8], fp: &FriParams, shift: &F, seed: &[u8; 32]) -> Result<bool, &'static str> {
    let mut ok = 0i32;
    let rc = unsafe {
        zk_fri_verify_host(F::ZK_FIELD, fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries, limbs(std::slice::from_ref(shift)),
                           seed.as_ptr(), proof.as_ptr(), proof.len() as u64, &mut ok)
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(ok != 0)
}
/// FRI polynomial commitment (include/zk_amd.h, zk_pcs_*; the reference has none): one commitment to `k` polynomials of at most
/// `2^log_degree` coefficients, opened at any number of points, one after another.
pub struct PolyCommitment<F: GpuField> { ctx: Rc<Ctx>, h: *mut zk_pcs, fp: FriParams, shift: F }
impl<F: GpuField> Drop for PolyCommitment<F> { fn drop(&mut self) { unsafe { zk_pcs_free(self.h); } } }
impl<F: GpuField> PolyCommitment<F> {
    /// Stream-ordered, no host wait; the handle does not refer to the polynomials afterwards.
    pub fn commit(polys: &[&UnivariatePolynomial<F>], log_degree: u32, log_blowup: u32, log_arity: u32, shift: &F) -> Result<Self, &'static str> {
        let c = ctx::<F>()?;
        let hs: Vec<*const zk_upoly> = polys.iter().map(|p| p.h as *const zk_upoly).collect();
        let mut h: *mut zk_pcs = std::ptr::null_mut();
        let rc = unsafe { zk_pcs_commit(c.raw, hs.as_ptr(), hs.len() as u32, log_degree, log_blowup, log_arity, limbs(std::slice::from_ref(shift)), &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self { ctx: c, h, fp: FriParams { log_degree, log_blowup, log_arity, log_final: 0, n_queries: 0 }, shift: *shift })
    }
    pub fn n_polys(&self) -> usize {
        let mut k = 0u32;
        unsafe { zk_pcs_n_polys(self.h, &mut k) };
        k as usize
    }
    pub fn root(&self) -> Result<[u8; 32], &'static str> {
        let mut d = [0u8; 32];
        let rc = unsafe { zk_pcs_root(self.ctx.raw, self.h, d.as_mut_ptr()) };
        if rc != 0 { return Err(err(rc)); }
        Ok(d)
    }
    pub fn shift(&self) -> F { self.shift }
    /// The values `f_c(z)` and the proof that they are right; the commitment is left intact.
    pub fn open(&self, z: &F, log_final: u32, n_queries: u32, seed: &[u8; 32]) -> Result<(Vec<F>, Vec<u8>), &'static str> {
        let k = self.n_polys();
        let fp = FriParams { log_final, n_queries, ..self.fp };
        let mut values = vec![F::zero(); k];
        let mut proof = vec![0u8; pcs_proof_bytes(k as u32, &fp)? as usize];
        let rc = unsafe {
            zk_pcs_open(self.ctx.raw, self.h, limbs(std::slice::from_ref(z)), log_final, n_queries, seed.as_ptr(), limbs_mut(&mut values), proof.as_mut_ptr())
        };
        if rc != 0 { return Err(err(rc)); }
        Ok((values, proof))
    }
}
pub fn pcs_proof_bytes(k: u32, fp: &FriParams) -> Result<u64, &'static str> {
    let mut n = 0u64;
    let rc = unsafe { zk_pcs_proof_bytes(k, fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries, &mut n) };
    if rc != 0 { return Err(err(rc)); }
    Ok(n)
}
/// Host only (zk_pcs_verify_host): needs no device.
pub fn pcs_verify<F: GpuField>(root: &[u8; 32], z: &F, values: &[F], proof: &[u8], fp: &FriParams, shift: &F, seed: &[u8; 32]) -> Result<bool, &'static str> {
    let mut ok = 0i32;
    let rc = unsafe {
        zk_pcs_verify_host(F::ZK_FIELD, values.len() as u32, fp.log_degree, fp.log_blowup, fp.log_arity, fp.log_final, fp.n_queries,
                           limbs(std::slice::from_ref(shift)), seed.as_ptr(), root.as_ptr(), limbs(std::slice::from_ref(z)), limbs(values),
                           proof.as_ptr(), proof.len() as u64, &mut ok)
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(ok != 0)
}
/// Multilinear polynomial commitment (include/zk_amd.h, zk_mlpcs_*; the reference has none): one commitment to a table, opened at any
/// number of points, one after another.
pub struct MultilinearCommitment<F: GpuField> { ctx: Rc<Ctx>, h: *mut zk_mlpcs, log_blowup: u32, shift: F }
impl<F: GpuField> Drop for MultilinearCommitment<F> { fn drop(&mut self) { unsafe { zk_mlpcs_free(self.h); } } }
impl<F: GpuField> MultilinearCommitment<F> {
    /// Stream-ordered, no host wait; the handle does not refer to the table afterwards.
    pub fn commit(table: &MultiLinearPolynomial<F>, log_blowup: u32, shift: &F) -> Result<Self, &'static str> {
        let mut h: *mut zk_mlpcs = std::ptr::null_mut();
        let rc = unsafe { zk_mlpcs_commit(table.ctx.raw, table.h as *const zk_mle, log_blowup, limbs(std::slice::from_ref(shift)), &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self { ctx: Rc::clone(&table.ctx), h, log_blowup, shift: *shift })
    }
    pub fn n_vars(&self) -> usize {
        let mut n = 0u32;
        unsafe { zk_mlpcs_n_vars(self.h, &mut n) };
        n as usize
    }
    pub fn root(&self) -> Result<[u8; 32], &'static str> {
        let mut d = [0u8; 32];
        let rc = unsafe { zk_mlpcs_root(self.ctx.raw, self.h, d.as_mut_ptr()) };
        if rc != 0 { return Err(err(rc)); }
        Ok(d)
    }
    pub fn shift(&self) -> F { self.shift }
    /// The value `t(point)` and the proof that it is right; the commitment is left intact.
    pub fn open(&self, point: &[F], log_final: u32, n_queries: u32, seed: &[u8; 32]) -> Result<(F, Vec<u8>), &'static str> {
        let mut value = [F::zero()];
        let mut proof = vec![0u8; mlpcs_proof_bytes(self.n_vars() as u32, self.log_blowup, log_final, n_queries)? as usize];
        let rc = unsafe {
            zk_mlpcs_open(self.ctx.raw, self.h, limbs(point), point.len() as u64, log_final, n_queries, seed.as_ptr(), limbs_mut(&mut value), proof.as_mut_ptr())
        };
        if rc != 0 { return Err(err(rc)); }
        Ok((value[0], proof))
    }
}
pub fn mlpcs_proof_bytes(n_vars: u32, log_blowup: u32, log_final: u32, n_queries: u32) -> Result<u64, &'static str> {
    let mut n = 0u64;
    let rc = unsafe { zk_mlpcs_proof_bytes(n_vars, log_blowup, log_final, n_queries, &mut n) };
    if rc != 0 { return Err(err(rc)); }
    Ok(n)
}
/// Host only (zk_mlpcs_verify_host): needs no device.
pub fn mlpcs_verify<F: GpuField>(root: &[u8; 32], point: &[F], value: &F, proof: &[u8], log_blowup: u32, log_final: u32, n_queries: u32, shift: &F,
                                 seed: &[u8; 32]) -> Result<bool, &'static str> {
    let mut ok = 0i32;
    let rc = unsafe {
        zk_mlpcs_verify_host(F::ZK_FIELD, point.len() as u32, log_blowup, log_final, n_queries, limbs(std::slice::from_ref(shift)), seed.as_ptr(),
                             root.as_ptr(), limbs(point), limbs(std::slice::from_ref(value)), proof.as_ptr(), proof.len() as u64, &mut ok)
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(ok != 0)
}
/// `S_X = sum_x' table[X 2^(n-1) + x'] eq(x', tail)`, `X = 0, 1` (zk_mle_eq_sums); `tail`: `n_vars - 1` elements.
pub fn eq_sums<F: GpuField>(table: &MultiLinearPolynomial<F>, tail: &[F]) -> Result<[F; 2], &'static str> {
    if tail.len() + 1 != table.n_vars as usize { return Err(err(ZK_ERR_BAD_ARG)); }
    let mut out = [F::zero(); 2];
    let rc = unsafe { zk_mle_eq_sums(table.ctx.raw, table.h as *const zk_mle, if tail.is_empty() { std::ptr::null() } else { limbs(tail) }, limbs_mut(&mut out)) };
    if rc != 0 { return Err(err(rc)); }
    Ok(out)
}
/// Batch multilinear commitment (include/zk_amd.h, zk_mlbatch_*; the reference has none): `k` tables of one size under one tree; every
/// opening shows all of them at `m` points with one proof.  Tables of another size go into another commitment.
pub struct MultilinearBatchCommitment<F: GpuField> { ctx: Rc<Ctx>, h: *mut zk_mlbatch, log_blowup: u32, shift: F }
impl<F: GpuField> Drop for MultilinearBatchCommitment<F> { fn drop(&mut self) { unsafe { zk_mlbatch_free(self.h); } } }
impl<F: GpuField> MultilinearBatchCommitment<F> {
    /// Stream-ordered, no host wait; the handle does not refer to the tables afterwards.
    pub fn commit(tables: &[&MultiLinearPolynomial<F>], log_blowup: u32, shift: &F) -> Result<Self, &'static str> {
        if tables.is_empty() { return Err(err(ZK_ERR_BAD_ARG)); }
        let hs: Vec<*const zk_mle> = tables.iter().map(|t| t.h as *const zk_mle).collect();
        let mut h: *mut zk_mlbatch = std::ptr::null_mut();
        let rc = unsafe { zk_mlbatch_commit(tables[0].ctx.raw, hs.as_ptr(), hs.len() as u32, log_blowup, limbs(std::slice::from_ref(shift)), &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self { ctx: Rc::clone(&tables[0].ctx), h, log_blowup, shift: *shift })
    }
    pub fn n_vars(&self) -> usize {
        let mut n = 0u32;
        unsafe { zk_mlbatch_n_vars(self.h, &mut n) };
        n as usize
    }
    pub fn n_tables(&self) -> usize {
        let mut k = 0u32;
        unsafe { zk_mlbatch_n_tables(self.h, &mut k) };
        k as usize
    }
    pub fn root(&self) -> Result<[u8; 32], &'static str> {
        let mut d = [0u8; 32];
        let rc = unsafe { zk_mlbatch_root(self.ctx.raw, self.h, d.as_mut_ptr()) };
        if rc != 0 { return Err(err(rc)); }
        Ok(d)
    }
    pub fn shift(&self) -> F { self.shift }
    /// `points`: `m * n_vars` elements, point after point.  The values `t_c(z_j)` (`m * k` elements, point-major) and the one proof of
    /// all of them; the commitment is left intact.
    pub fn open(&self, points: &[F], log_final: u32, n_queries: u32, seed: &[u8; 32]) -> Result<(Vec<F>, Vec<u8>), &'static str> {
        let (n, k) = (self.n_vars(), self.n_tables());
        if points.is_empty() || points.len() % n != 0 { return Err(err(ZK_ERR_BAD_ARG)); }
        let m = points.len() / n;
        let mut values = vec![F::zero(); m * k];
        let mut proof = vec![0u8; mlbatch_proof_bytes(n as u32, k as u32, m as u32, self.log_blowup, log_final, n_queries)? as usize];
        let rc = unsafe {
            zk_mlbatch_open(self.ctx.raw, self.h, limbs(points), m as u32, log_final, n_queries, seed.as_ptr(), limbs_mut(&mut values), proof.as_mut_ptr())
        };
        if rc != 0 { return Err(err(rc)); }
        Ok((values, proof))
    }
}
pub fn mlbatch_proof_bytes(n_vars: u32, n_tables: u32, n_points: u32, log_blowup: u32, log_final: u32, n_queries: u32) -> Result<u64, &'static str> {
    let mut n = 0u64;
    let rc = unsafe { zk_mlbatch_proof_bytes(n_vars, n_tables, n_points, log_blowup, log_final, n_queries, &mut n) };
    if rc != 0 { return Err(err(rc)); }
    Ok(n)
}
/// Host only (zk_mlbatch_verify_host): needs no device.  `points`: `m * n_vars` elements, `values`: `m * k`, both point-major.
pub fn mlbatch_verify<F: GpuField>(root: &[u8; 32], n_vars: usize, points: &[F], values: &[F], proof: &[u8], log_blowup: u32, log_final: u32,
                                   n_queries: u32, shift: &F, seed: &[u8; 32]) -> Result<bool, &'static str> {
    if n_vars == 0 || points.is_empty() || points.len() % n_vars != 0 { return Err(err(ZK_ERR_BAD_ARG)); }
    let m = points.len() / n_vars;
    if values.is_empty() || values.len() % m != 0 { return Err(err(ZK_ERR_BAD_ARG)); }
    let mut ok = 0i32;
    let rc = unsafe {
        zk_mlbatch_verify_host(F::ZK_FIELD, n_vars as u32, (values.len() / m) as u32, m as u32, log_blowup, log_final, n_queries,
                               limbs(std::slice::from_ref(shift)), seed.as_ptr(), root.as_ptr(), limbs(points), limbs(values), proof.as_ptr(),
                               proof.len() as u64, &mut ok)
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(ok != 0)
}
/// `sum_c coeffs[c] tables[c]` as a new table (zk_mle_lincomb).
pub fn lincomb<F: GpuField>(tables: &[&MultiLinearPolynomial<F>], coeffs: &[F]) -> Result<MultiLinearPolynomial<F>, &'static str> {
    if tables.is_empty() || coeffs.len() != tables.len() { return Err(err(ZK_ERR_BAD_ARG)); }
    let hs: Vec<*const zk_mle> = tables.iter().map(|t| t.h as *const zk_mle).collect();
    let mut h: *mut zk_mle = std::ptr::null_mut();
    let rc = unsafe { zk_mle_alloc(tables[0].ctx.raw, tables[0].n_vars as u64, &mut h) };
    if rc != 0 { return Err(err(rc)); }
    let out = MultiLinearPolynomial::from_handle(Rc::clone(&tables[0].ctx), h);
    let rc = unsafe { zk_mle_lincomb(tables[0].ctx.raw, hs.as_ptr(), hs.len() as u32, limbs(coeffs), out.h) };
    if rc != 0 { return Err(err(rc)); }
    Ok(out)
}
/// `eq_sums` at `m` tails in passes of several points over the table (zk_mle_eq_sums_many); `tails`: `m * (n_vars - 1)` elements; the
/// result holds `(S_0^j, S_1^j)` point after point.
pub fn eq_sums_many<F: GpuField>(table: &MultiLinearPolynomial<F>, tails: &[F], n_points: usize) -> Result<Vec<[F; 2]>, &'static str> {
    if n_points == 0 || table.n_vars == 0 || tails.len() != n_points * (table.n_vars as usize - 1) { return Err(err(ZK_ERR_BAD_ARG)); }
    let mut out = vec![F::zero(); 2 * n_points];
    let rc = unsafe {
        zk_mle_eq_sums_many(table.ctx.raw, table.h as *const zk_mle, if tails.is_empty() { std::ptr::null() } else { limbs(tails) }, n_points as u32,
                            limbs_mut(&mut out))
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(out.chunks(2).map(|p| [p[0], p[1]]).collect())
}
/// Grand-product argument (include/zk_amd.h, zk_mle_product_tree / zk_gprod_*; the reference has none): `P = prod_i (t[i] + shift)` shown
/// to a verifier who is left with the one claim `t(point) = claim`.  The seed must bind the table (e.g. its commitment's root).
pub struct GrandProductProof<F: GpuField> { pub product: F, pub proof: Vec<u8>, pub point: Vec<F>, pub claim: F }
fn shift_ptr<F: GpuField>(shift: Option<&F>) -> *const u64 {
    match shift { Some(s) => limbs(std::slice::from_ref(s)), None => std::ptr::null() }
}
pub fn gprod_proof_bytes(n_vars: u32) -> Result<u64, &'static str> {
    let mut n = 0u64;
    let rc = unsafe { zk_gprod_proof_bytes(n_vars, &mut n) };
    if rc != 0 { return Err(err(rc)); }
    Ok(n)
}
/// The product tree over `table + shift` in heap order: `out[0] = 1`, `out[2^j + i] = V_j[i]`, `out[1] = P`.  Stream-ordered, no host wait.
pub fn product_tree<F: GpuField>(table: &MultiLinearPolynomial<F>, shift: Option<&F>) -> Result<MultiLinearPolynomial<F>, &'static str> {
    let mut h: *mut zk_mle = std::ptr::null_mut();
    let rc = unsafe { zk_mle_product_tree(table.ctx.raw, table.h as *const zk_mle, shift_ptr(shift), &mut h) };
    if rc != 0 { return Err(err(rc)); }
    Ok(MultiLinearPolynomial::from_handle(Rc::clone(&table.ctx), h))
}
/// One host wait for the whole proof; the table is left intact.
pub fn grand_product_prove<F: GpuField>(table: &MultiLinearPolynomial<F>, seed: &[u8; 32], shift: Option<&F>) -> Result<GrandProductProof<F>, &'static str> {
    let n = table.n_vars as usize;
    let mut proof = vec![0u8; gprod_proof_bytes(n as u32)? as usize];
    let (mut product, mut claim, mut point) = ([F::zero()], [F::zero()], vec![F::zero(); n]);
    let rc = unsafe {
        zk_gprod_prove(table.ctx.raw, table.h as *const zk_mle, shift_ptr(shift), seed.as_ptr(), limbs_mut(&mut product), proof.as_mut_ptr(),
                       limbs_mut(&mut point), limbs_mut(&mut claim))
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(GrandProductProof { product: product[0], proof, point, claim: claim[0] })
}
/// Host only (zk_gprod_verify_host): needs no device.  `Some((point, claim))`: what is left to check is `t(point) == claim`.
pub fn grand_product_verify<F: GpuField>(n_vars: u32, seed: &[u8; 32], product: &F, proof: &[u8], shift: Option<&F>) -> Result<Option<(Vec<F>, F)>, &'static str> {
    let (mut ok, mut claim, mut point) = (0i32, [F::zero()], vec![F::zero(); std::cmp::max(n_vars as usize, 1)]);
    let rc = unsafe {
        zk_gprod_verify_host(F::ZK_FIELD, n_vars, shift_ptr(shift), seed.as_ptr(), limbs(std::slice::from_ref(product)), proof.as_ptr(), proof.len() as u64,
                             limbs_mut(&mut point), limbs_mut(&mut claim), &mut ok)
    };
    if rc != 0 { return Err(err(rc)); }
    point.truncate(n_vars as usize);
    Ok(if ok != 0 { Some((point, claim[0])) } else { None })
}
/// Zerocheck argument (include/zk_amd.h, zk_gate_* / zk_zerocheck_*; the reference has none): `G(t_0[i], .., t_{k-1}[i]) = 0` on every row
/// for the gate `G = sum_i coeff_i prod_{f in term i} x_f`, shown to a verifier who is left with the `k` claims `t_c(point) = claims[c]`.
/// The seed must bind the tables (e.g. their batch commitment's root).  A gate is a host object and needs no device.
pub struct Gate<F: GpuField> { h: *mut zk_gate, k: u32, d: u32, _f: std::marker::PhantomData<F> }
impl<F: GpuField> Gate<F> {
    /// `terms`: `(coefficient, column indices)`; a repeated column is a power, no column a constant.
    pub fn new(k: u32, terms: &[(F, Vec<u32>)]) -> Result<Self, &'static str> {
        if terms.is_empty() { return Err(err(ZK_ERR_BAD_ARG)); }
        let coeffs: Vec<F> = terms.iter().map(|t| t.0).collect();
        let lens: Vec<u32> = terms.iter().map(|t| t.1.len() as u32).collect();
        let mut flat: Vec<u32> = terms.iter().flat_map(|t| t.1.iter().copied()).collect();
        if flat.is_empty() { flat.push(0); }
        let mut h: *mut zk_gate = std::ptr::null_mut();
        let rc = unsafe { zk_gate_create(F::ZK_FIELD, k, terms.len() as u32, limbs(&coeffs), lens.as_ptr(), flat.as_ptr(), &mut h) };
        if rc != 0 { return Err(err(rc)); }
        let (mut d, mut kk) = (0u32, 0u32);
        let rc = unsafe { zk_gate_degree(h, &mut d) | zk_gate_n_columns(h, &mut kk) };
        assert!(rc == 0 && kk == k);
        Ok(Gate { h, k, d, _f: std::marker::PhantomData })
    }
    pub fn degree(&self) -> u32 { self.d }
    pub fn n_columns(&self) -> u32 { self.k }
}
impl<F: GpuField> Drop for Gate<F> {
    fn drop(&mut self) { unsafe { zk_gate_free(self.h); } }
}
pub struct ZerocheckProof<F: GpuField> { pub proof: Vec<u8>, pub point: Vec<F>, pub claims: Vec<F> }
pub fn zerocheck_proof_bytes<F: GpuField>(gate: &Gate<F>, n_vars: u32) -> Result<u64, &'static str> {
    let mut n = 0u64;
    let rc = unsafe { zk_zerocheck_proof_bytes(gate.h, n_vars, &mut n) };
    if rc != 0 { return Err(err(rc)); }
    Ok(n)
}
/// One host wait for the whole proof; the tables are left intact.  The prover does not check the statement.
pub fn zerocheck_prove<F: GpuField>(tables: &[&MultiLinearPolynomial<F>], gate: &Gate<F>, seed: &[u8; 32]) -> Result<ZerocheckProof<F>, &'static str> {
    if tables.len() != gate.k as usize { return Err(err(ZK_ERR_BAD_ARG)); }
    let n = tables[0].n_vars as usize;
    let hs: Vec<*const zk_mle> = tables.iter().map(|t| t.h as *const zk_mle).collect();
    let mut proof = vec![0u8; zerocheck_proof_bytes(gate, n as u32)? as usize];
    let (mut point, mut claims) = (vec![F::zero(); std::cmp::max(n, 1)], vec![F::zero(); gate.k as usize]);
    let rc = unsafe { zk_zerocheck_prove(tables[0].ctx.raw, hs.as_ptr(), gate.h, seed.as_ptr(), proof.as_mut_ptr(), limbs_mut(&mut point), limbs_mut(&mut claims)) };
    if rc != 0 { return Err(err(rc)); }
    point.truncate(n);
    Ok(ZerocheckProof { proof, point, claims })
}
/// Host only (zk_zerocheck_verify_host): needs no device.  `Some((point, claims))`: what is left to check is `t_c(point) == claims[c]`.
pub fn zerocheck_verify<F: GpuField>(gate: &Gate<F>, n_vars: u32, seed: &[u8; 32], proof: &[u8]) -> Result<Option<(Vec<F>, Vec<F>)>, &'static str> {
    let (mut ok, mut claims, mut point) = (0i32, vec![F::zero(); gate.k as usize], vec![F::zero(); std::cmp::max(n_vars as usize, 1)]);
    let rc = unsafe { zk_zerocheck_verify_host(gate.h, n_vars, seed.as_ptr(), proof.as_ptr(), proof.len() as u64, limbs_mut(&mut point), limbs_mut(&mut claims), &mut ok) };
    if rc != 0 { return Err(err(rc)); }
    point.truncate(n_vars as usize);
    Ok(if ok != 0 { Some((point, claims)) } else { None })
}
/// `sum_x' eq(x', tail) G(tables(X, x'))` at `X = 0 .. d` (zk_mle_gate_sums), the tables as they are; `tail`: `n_vars - 1` elements.
pub fn gate_sums<F: GpuField>(tables: &[&MultiLinearPolynomial<F>], gate: &Gate<F>, tail: &[F]) -> Result<Vec<F>, &'static str> {
    if tables.len() != gate.k as usize || tail.len() + 1 != tables[0].n_vars as usize { return Err(err(ZK_ERR_BAD_ARG)); }
    let hs: Vec<*const zk_mle> = tables.iter().map(|t| t.h as *const zk_mle).collect();
    let mut out = vec![F::zero(); gate.d as usize + 1];
    let rc = unsafe { zk_mle_gate_sums(tables[0].ctx.raw, hs.as_ptr(), gate.h, if tail.is_empty() { std::ptr::null() } else { limbs(tail) }, limbs_mut(&mut out)) };
    if rc != 0 { return Err(err(rc)); }
    Ok(out)
}
/// Wiring (copy-constraint) permutation argument (include/zk_amd.h, zk_perm_*; the reference has none): the witness columns `w` satisfy
/// the wiring `sigma` (`sigma_c[i]` = the label `c' 2^n + i'` of the cell that `(c, i)` is wired to), shown to a verifier who is left with
/// the `2 k` claims `w_c(point) = claims[c]`, `sigma_c(point) = claims[k + c]` at one point.  The seed must bind the commitments of `w` and
/// `sigma`, and `beta`, `gamma` must be drawn after that; that `sigma` is a permutation is the circuit's preprocessing to guarantee.
pub struct PermutationProof<F: GpuField> { pub proof: Vec<u8>, pub point: Vec<F>, pub claims: Vec<F> }
pub fn perm_proof_bytes(n_vars: u32, k: u32) -> Result<u64, &'static str> {
    let mut n = 0u64;
    let rc = unsafe { zk_perm_proof_bytes(n_vars, k, &mut n) };
    if rc != 0 { return Err(err(rc)); }
    Ok(n)
}
/// Two host waits (the grand product, then the `2 k` values); the columns are left intact.  The prover does not check the statement.
pub fn permutation_prove<F: GpuField>(w: &[&MultiLinearPolynomial<F>], sigma: &[&MultiLinearPolynomial<F>], beta: &F, gamma: &F, seed: &[u8; 32])
    -> Result<PermutationProof<F>, &'static str> {
    if w.is_empty() || w.len() != sigma.len() { return Err(err(ZK_ERR_BAD_ARG)); }
    let (n, k) = (w[0].n_vars as usize, w.len());
    let ws: Vec<*const zk_mle> = w.iter().map(|t| t.h as *const zk_mle).collect();
    let ss: Vec<*const zk_mle> = sigma.iter().map(|t| t.h as *const zk_mle).collect();
    let mut proof = vec![0u8; perm_proof_bytes(n as u32, k as u32)? as usize];
    let (mut point, mut claims) = (vec![F::zero(); std::cmp::max(n, 1)], vec![F::zero(); 2 * k]);
    let rc = unsafe { zk_perm_prove(w[0].ctx.raw, ws.as_ptr(), ss.as_ptr(), k as u32, limbs(std::slice::from_ref(beta)), limbs(std::slice::from_ref(gamma)),
                                    seed.as_ptr(), proof.as_mut_ptr(), limbs_mut(&mut point), limbs_mut(&mut claims)) };
    if rc != 0 { return Err(err(rc)); }
    point.truncate(n);
    Ok(PermutationProof { proof, point, claims })
}
/// Host only (zk_perm_verify_host): needs no device.  `Some((point, claims))`: what is left to check is the `2 k` evaluations.
pub fn permutation_verify<F: GpuField>(n_vars: u32, k: u32, beta: &F, gamma: &F, seed: &[u8; 32], proof: &[u8]) -> Result<Option<(Vec<F>, Vec<F>)>, &'static str> {
    if k < 1 || k > 16 { return Err(err(ZK_ERR_BAD_ARG)); }
    let (mut ok, mut claims, mut point) = (0i32, vec![F::zero(); 2 * k as usize], vec![F::zero(); std::cmp::max(n_vars as usize, 1)]);
    let rc = unsafe { zk_perm_verify_host(F::ZK_FIELD, n_vars, k, limbs(std::slice::from_ref(beta)), limbs(std::slice::from_ref(gamma)), seed.as_ptr(),
                                          proof.as_ptr(), proof.len() as u64, limbs_mut(&mut point), limbs_mut(&mut claims), &mut ok) };
    if rc != 0 { return Err(err(rc)); }
    point.truncate(n_vars as usize);
    Ok(if ok != 0 { Some((point, claims)) } else { None })
}
/// Fractional-sum (LogUp) argument (include/zk_amd.h, zk_mle_fraction_tree / zk_fsum_*; the reference has none): `N / D = sum_i p[i] /
/// (q[i] + shift)` shown to a verifier who is left with the two claims `p(point) = claims[0]`, `q(point) = claims[1]`.  `p = None`: all
/// ones.  The seed must bind the tables (e.g. their commitments' roots).
pub struct FractionalSumProof<F: GpuField> { pub sum: [F; 2], pub proof: Vec<u8>, pub point: Vec<F>, pub claims: [F; 2] }
fn mle_ptr<F: GpuField>(t: Option<&MultiLinearPolynomial<F>>) -> *const zk_mle {
    match t { Some(t) => t.h as *const zk_mle, None => std::ptr::null() }
}
pub fn fsum_proof_bytes(n_vars: u32) -> Result<u64, &'static str> {
    let mut n = 0u64;
    let rc = unsafe { zk_fsum_proof_bytes(n_vars, &mut n) };
    if rc != 0 { return Err(err(rc)); }
    Ok(n)
}
/// Both heaps of the fraction tree, `(P, Q)`: `out[2^j + i]` = level j, `P[1] = N`, `Q[1] = D`.  Stream-ordered, no host wait.
pub fn fraction_tree<F: GpuField>(p: Option<&MultiLinearPolynomial<F>>, q: &MultiLinearPolynomial<F>, shift: Option<&F>)
                                  -> Result<(MultiLinearPolynomial<F>, MultiLinearPolynomial<F>), &'static str> {
    let (mut hp, mut hq): (*mut zk_mle, *mut zk_mle) = (std::ptr::null_mut(), std::ptr::null_mut());
    let rc = unsafe { zk_mle_fraction_tree(q.ctx.raw, mle_ptr(p), q.h as *const zk_mle, shift_ptr(shift), &mut hp, &mut hq) };
    if rc != 0 { return Err(err(rc)); }
    Ok((MultiLinearPolynomial::from_handle(Rc::clone(&q.ctx), hp), MultiLinearPolynomial::from_handle(Rc::clone(&q.ctx), hq)))
}
/// One host wait for the whole proof; the tables are left intact.
pub fn fractional_sum_prove<F: GpuField>(p: Option<&MultiLinearPolynomial<F>>, q: &MultiLinearPolynomial<F>, seed: &[u8; 32], shift: Option<&F>)
                                         -> Result<FractionalSumProof<F>, &'static str> {
    let n = q.n_vars as usize;
    let mut proof = vec![0u8; fsum_proof_bytes(n as u32)? as usize];
    let (mut sum, mut claims, mut point) = ([F::zero(); 2], [F::zero(); 2], vec![F::zero(); n]);
    let rc = unsafe {
        zk_fsum_prove(q.ctx.raw, mle_ptr(p), q.h as *const zk_mle, shift_ptr(shift), seed.as_ptr(), limbs_mut(&mut sum), proof.as_mut_ptr(),
                      limbs_mut(&mut point), limbs_mut(&mut claims))
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(FractionalSumProof { sum, proof, point, claims })
}
/// Host only (zk_fsum_verify_host): needs no device.  `Some((point, claims))`: what is left to check is `p(point) == claims[0]` (checked
/// here to be 1 when `has_p` is false) and `q(point) == claims[1]`.  `D = 0` is rejected.
pub fn fractional_sum_verify<F: GpuField>(n_vars: u32, has_p: bool, seed: &[u8; 32], sum: &[F; 2], proof: &[u8], shift: Option<&F>)
                                          -> Result<Option<(Vec<F>, [F; 2])>, &'static str> {
    let (mut ok, mut claims, mut point) = (0i32, [F::zero(); 2], vec![F::zero(); std::cmp::max(n_vars as usize, 1)]);
    let rc = unsafe {
        zk_fsum_verify_host(F::ZK_FIELD, n_vars, has_p as i32, shift_ptr(shift), seed.as_ptr(), limbs(sum), proof.as_ptr(), proof.len() as u64,
                            limbs_mut(&mut point), limbs_mut(&mut claims), &mut ok)
    };
    if rc != 0 { return Err(err(rc)); }
    point.truncate(n_vars as usize);
    Ok(if ok != 0 { Some((point, claims)) } else { None })
}
/// `(m, missing, first_missing, duplicates)` of zk_lookup_multiplicities: `m[j] = #{i : witness[i] = table[j]}` for the lowest `j` of
/// each value, else 0; `first_missing = u64::MAX`: every witness entry is in the table.
pub fn lookup_multiplicities<F: GpuField>(table: &MultiLinearPolynomial<F>, witness: &MultiLinearPolynomial<F>)
                                          -> Result<(MultiLinearPolynomial<F>, u64, u64, u64), &'static str> {
    let mut h: *mut zk_mle = std::ptr::null_mut();
    let (mut missing, mut first, mut dup) = (0u64, 0u64, 0u64);
    let rc = unsafe { zk_lookup_multiplicities(table.ctx.raw, table.h as *const zk_mle, witness.h as *const zk_mle, &mut h, &mut missing, &mut first, &mut dup) };
    if rc != 0 { return Err(err(rc)); }
    Ok((MultiLinearPolynomial::from_handle(Rc::clone(&table.ctx), h), missing, first, dup))
}
/// `out[i] = (sum_c alpha^c (columns[c][i] - values[c])) / (shift w^i - z)` over the columns' coset, as a new table (zk_deep_quotient).
pub fn deep_quotient<F: GpuField>(columns: &[&MultiLinearPolynomial<F>], shift: &F, z: &F, values: &[F], alpha: &F) -> Result<MultiLinearPolynomial<F>, &'static str> {
    if columns.is_empty() || values.len() != columns.len() { return Err(err(ZK_ERR_BAD_ARG)); }
    let hs: Vec<*const zk_mle> = columns.iter().map(|t| t.h as *const zk_mle).collect();
    let mut h: *mut zk_mle = std::ptr::null_mut();
    let rc = unsafe { zk_mle_alloc(columns[0].ctx.raw, columns[0].n_vars as u64, &mut h) };
    if rc != 0 { return Err(err(rc)); }
    let out = MultiLinearPolynomial::from_handle(Rc::clone(&columns[0].ctx), h);
    let rc = unsafe {
        zk_deep_quotient(columns[0].ctx.raw, hs.as_ptr(), hs.len() as u32, limbs(std::slice::from_ref(shift)), limbs(std::slice::from_ref(z)), limbs(values),
                         limbs(std::slice::from_ref(alpha)), out.h)
    };
    if rc != 0 { return Err(err(rc)); }
    Ok(out)
}
/// univariate_poly.rs:157-184 — `&a + &b`; an empty operand gives a copy of the other, otherwise max(la, lb) coefficients
impl<F: GpuField> std::ops::Add for &UnivariatePolynomial<F> {
    type Output = UnivariatePolynomial<F>;
    fn add(self, other: Self) -> Self::Output {
        let mut h: *mut zk_upoly = std::ptr::null_mut();
        let rc = unsafe { zk_upoly_add(self.ctx.raw, self.h, other.h, &mut h) };
        assert!(rc == 0, "{}", err(rc));
        UnivariatePolynomial::from_handle(Rc::clone(&self.ctx), h)
    }
}
/// univariate_poly.rs:186-209 — `&a * &b`; an empty operand gives the empty polynomial, otherwise la + lb - 1 coefficients
impl<F: GpuField> std::ops::Mul for &UnivariatePolynomial<F> {
    type Output = UnivariatePolynomial<F>;
    fn mul(self, other: Self) -> Self::Output {
        let mut h: *mut zk_upoly = std::ptr::null_mut();
        let rc = unsafe { zk_upoly_mul(self.ctx.raw, self.h, other.h, &mut h) };
        assert!(rc == 0, "{}", err(rc));
        UnivariatePolynomial::from_handle(Rc::clone(&self.ctx), h)
    }
}

/// polynomial::multilinear::coefficient_form::CoeffMultilinearPolynomial (coefficient_form.rs:27-30), resident in HBM, for the key
/// sets the dense form can carry: `interpolate` and `new_dense` make every key 0 .. 2^n_vars - 1 present; `partial_evaluate` removes
/// exactly the keys with a bit of a fixed variable, so the present keys are always {k : k & fixed_mask() == 0} and the object holds
/// their coefficients in ascending key order.  `Add` and `Mul` need `fixed_mask() == 0` (relabel first).  One divergence, in `Mul`
/// only: the reference skips pairs with a zero coefficient (:393-395) and so leaves their keys out of the product; here those keys
/// are present with coefficient zero (equal as polynomials; key for key equal when no operand coefficient is zero).
pub struct CoeffMultilinearPolynomial<F: GpuField> {
    ctx: Rc<Ctx>,
    h: *mut zk_cmle,
    _f: PhantomData<F>,
}
impl<F: GpuField> Drop for CoeffMultilinearPolynomial<F> {
    fn drop(&mut self) { unsafe { zk_cmle_free(self.ctx.raw, self.h); } }
}
/// #[derive(Clone)] coefficient_form.rs:16 — a device-side copy (partial_evaluate of nothing, :85)
impl<F: GpuField> Clone for CoeffMultilinearPolynomial<F> {
    fn clone(&self) -> Self { self.partial_evaluate(&[]).unwrap_or_else(|e| panic!("{}", e)) }
}
/// #[derive(PartialEq)] coefficient_form.rs:16 — n_vars and the map: the same keys with the same coefficients
impl<F: GpuField> PartialEq for CoeffMultilinearPolynomial<F> {
    fn eq(&self, other: &Self) -> bool {
        self.n_vars() == other.n_vars() && self.fixed_mask() == other.fixed_mask() && self.dense() == other.dense()
    }
}
/// #[derive(Debug)] coefficient_form.rs:16
impl<F: GpuField> fmt::Debug for CoeffMultilinearPolynomial<F> {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        f.debug_struct("CoeffMultilinearPolynomial").field("n_vars", &self.n_vars()).field("coefficients", &self.coefficients()).finish()
    }
}
impl<F: GpuField> CoeffMultilinearPolynomial<F> {
    fn from_handle(ctx: Rc<Ctx>, h: *mut zk_cmle) -> Self { Self { ctx, h, _f: PhantomData } }
    /// All 2^n_vars coefficients, index = key (zeros included): Err when the length is not 2^n_vars.
    pub fn new_dense(n_vars: u32, coefficients: &[F]) -> Result<Self, &'static str> {
        let c = ctx::<F>()?;
        let mut h: *mut zk_cmle = std::ptr::null_mut();
        let rc = unsafe { zk_cmle_upload(c.raw, n_vars as u64, limbs(coefficients), coefficients.len() as u64, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self::from_handle(c, h))
    }
    /// coefficient_form.rs:200-216 of a resident table (one value: n_vars 1)
    pub fn interpolate(values: &MultiLinearPolynomial<F>) -> Self {
        let mut h: *mut zk_cmle = std::ptr::null_mut();
        let rc = unsafe { zk_cmle_interpolate(values.ctx.raw, values.h, &mut h) };
        assert!(rc == 0, "{}", err(rc));
        Self::from_handle(Rc::clone(&values.ctx), h)
    }
    /// coefficient_form.rs:34-36
    pub fn n_vars(&self) -> usize {
        let mut n = 0u64;
        unsafe { zk_cmle_n_vars(self.h, &mut n); }
        n as usize
    }
    /// bit v set <-> variable v has been fixed by partial_evaluate: no present key has bit v
    pub fn fixed_mask(&self) -> u64 {
        let mut m = 0u64;
        unsafe { zk_cmle_fixed_mask(self.h, &mut m); }
        m
    }
    /// the coefficients of the present keys, ascending key order (downloads)
    fn dense(&self) -> Vec<F> {
        let mut n = 0u64;
        unsafe { zk_cmle_len(self.h, &mut n); }
        let mut v = vec![F::zero(); n as usize];
        let rc = unsafe { zk_cmle_download(self.ctx.raw, self.h, limbs_mut(&mut v)) };
        assert!(rc == 0, "{}", err(rc));
        v
    }
    /// coefficient_form.rs:195-197 — the map of the present keys (downloads): entry j of the stored vector is the key whose bits,
    /// at the positions not in fixed_mask() from the lowest up, are the bits of j
    pub fn coefficients(&self) -> std::collections::BTreeMap<usize, F> {
        let (fixed, n) = (self.fixed_mask(), self.n_vars());
        self.dense().into_iter().enumerate().map(|(j, coeff)| {
            let (mut key, mut at) = (0usize, 0usize);
            for v in 0..n {
                if fixed >> v & 1 == 0 {
                    key |= ((j >> at) & 1) << v;
                    at += 1;
                }
            }
            (key, coeff)
        }).collect()
    }
    /// coefficient_form.rs:72-104 — the reference's signature; its two selector errors come back as its own texts
    pub fn partial_evaluate(&self, assignments: &[(Vec<bool>, &F)]) -> Result<Self, &'static str> {
        let lens: Vec<u64> = assignments.iter().map(|(s, _)| s.len() as u64).collect();
        let sel: Vec<u8> = assignments.iter().flat_map(|(s, _)| s.iter().map(|b| *b as u8)).collect();
        let vals: Vec<F> = assignments.iter().map(|(_, v)| **v).collect();
        let mut h: *mut zk_cmle = std::ptr::null_mut();
        let rc = unsafe { zk_cmle_partial_evaluate(self.ctx.raw, self.h, sel.as_ptr(), lens.as_ptr(), limbs(&vals), assignments.len() as u64,
                                                   &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(Self::from_handle(Rc::clone(&self.ctx), h))
    }
    /// coefficient_form.rs:109-123 — consumes self like the reference; no device work (the stored vector is already the relabelled one)
    pub fn relabel(self) -> Self {
        let rc = unsafe { zk_cmle_relabel(self.ctx.raw, self.h) };
        assert!(rc == 0, "{}", err(rc));
        self
    }
    /// coefficient_form.rs:272-282
    pub fn scalar_multiply(&self, scalar: &F) -> Self {
        let mut h: *mut zk_cmle = std::ptr::null_mut();
        let rc = unsafe { zk_cmle_scalar_multiply(self.ctx.raw, self.h, limbs(std::slice::from_ref(scalar)), &mut h) };
        assert!(rc == 0, "{}", err(rc));
        Self::from_handle(Rc::clone(&self.ctx), h)
    }
    /// coefficient_form.rs:39-69
    pub fn evaluate_slice(&self, assignments: &[F]) -> Result<F, &'static str> {
        let mut out = [F::zero()];
        let rc = unsafe { zk_cmle_evaluate(self.ctx.raw, self.h, limbs(assignments), assignments.len() as u64, limbs_mut(&mut out)) };
        if rc != 0 { return Err(err(rc)); } // "evaluate requires an assignment for every variable"
        Ok(out[0])
    }
    /// coefficient_form.rs:340-347, left resident; Err on a partially evaluated polynomial until it is relabelled
    pub fn to_evaluation_form(&self) -> Result<MultiLinearPolynomial<F>, &'static str> {
        let mut h: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_cmle_to_evaluation(self.ctx.raw, self.h, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(MultiLinearPolynomial::from_handle(Rc::clone(&self.ctx), h))
    }
    /// coefficient_form.rs:131-139
    pub fn to_bytes(&self) -> Vec<u8> {
        let mut n = 0u64;
        unsafe { zk_cmle_len(self.h, &mut n); }
        let mut b = vec![0u8; 4 + 40 * n as usize];
        let rc = unsafe { zk_cmle_to_bytes(self.ctx.raw, self.h, b.as_mut_ptr()) };
        assert!(rc == 0, "{}", err(rc));
        b
    }
}
/// coefficient_form.rs:350-373 — `&a + &b`, a Result like the reference's; Err when an operand is partially evaluated (relabel first)
impl<F: GpuField> std::ops::Add for &CoeffMultilinearPolynomial<F> {
    type Output = Result<CoeffMultilinearPolynomial<F>, &'static str>;
    fn add(self, rhs: Self) -> Self::Output {
        let mut h: *mut zk_cmle = std::ptr::null_mut();
        let rc = unsafe { zk_cmle_add(self.ctx.raw, self.h, rhs.h, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        Ok(CoeffMultilinearPolynomial::from_handle(Rc::clone(&self.ctx), h))
    }
}
/// coefficient_form.rs:375-415 — `&a * &b`, the lhs variables first; panics with the library's message where the product cannot be
/// formed (a partially evaluated operand, more than 40 variables)
impl<F: GpuField> std::ops::Mul for &CoeffMultilinearPolynomial<F> {
    type Output = CoeffMultilinearPolynomial<F>;
    fn mul(self, rhs: Self) -> Self::Output {
        let mut h: *mut zk_cmle = std::ptr::null_mut();
        let rc = unsafe { zk_cmle_mul(self.ctx.raw, self.h, rhs.h, &mut h) };
        assert!(rc == 0, "{}", err(rc));
        CoeffMultilinearPolynomial::from_handle(Rc::clone(&self.ctx), h)
    }
}

/// polynomial::product_poly::ProductPoly (product_poly.rs:6-10)
#[derive(Clone, Debug, PartialEq)]
pub struct ProductPoly<F: GpuField> { n_vars: usize, polynomials: Vec<MultiLinearPolynomial<F>> }

impl<F: GpuField> ProductPoly<F> {
    fn handles(&self) -> Vec<*const zk_mle> { self.polynomials.iter().map(|p| p.h as *const zk_mle).collect() }
    fn ctx_raw(&self) -> *mut zk_ctx { self.polynomials[0].ctx.raw }
    /// product_poly.rs:14-32
    pub fn new(polynomials: Vec<MultiLinearPolynomial<F>>) -> Result<Self, &'static str> {
        let h: Vec<*const zk_mle> = polynomials.iter().map(|p| p.h as *const zk_mle).collect();
        let rc = unsafe { zk_product_check(h.as_ptr(), h.len() as u64) };
        if rc != 0 { return Err(err(rc)); } // the two Err texts of product_poly.rs:16,25
        Ok(Self { n_vars: polynomials[0].n_vars(), polynomials })
    }
    /// product_poly.rs:86
    pub fn n_vars(&self) -> usize { self.n_vars }
    /// product_poly.rs:36-44
    pub fn evaluate(&self, assignments: &[F]) -> Result<F, &'static str> {
        let h = self.handles();
        let mut out = [F::zero()];
        let rc = unsafe { zk_product_evaluate(self.ctx_raw(), h.as_ptr(), h.len() as u64, limbs(assignments),
                                              assignments.len() as u64, limbs_mut(&mut out)) };
        if rc != 0 { return Err(err(rc)); }
        Ok(out[0])
    }
    /// product_poly.rs:48-63
    pub fn partial_evaluate(&self, initial_var: usize, assignments: &[F]) -> Result<Self, &'static str> {
        let polynomials = self.polynomials.iter().map(|p| p.partial_evaluate(initial_var, assignments))
            .collect::<Result<Vec<_>, _>>()?;
        Ok(Self { n_vars: polynomials[0].n_vars(), polynomials })
    }
    /// product_poly.rs:66-74
    pub fn prod_reduce(&self) -> Vec<F> {
        let h = self.handles();
        let mut o: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_prod_reduce(self.ctx_raw(), h.as_ptr(), h.len() as u64, &mut o) };
        assert!(rc == 0, "{}", err(rc));
        MultiLinearPolynomial::<F>::from_handle(Rc::clone(&self.polynomials[0].ctx), o).evaluation_slice().to_vec()
    }
    /// product_poly.rs:77-83
    pub fn to_bytes(&self) -> Vec<u8> { self.polynomials.iter().flat_map(|p| p.to_bytes()).collect() }
}

/// transcript::Transcript (transcript/src/lib.rs:5-35): Keccak-256 sponge, host side.
pub struct Transcript { h: *mut zk_transcript }
impl Drop for Transcript {
    fn drop(&mut self) { unsafe { zk_transcript_free(self.h); } }
}
impl Transcript {
    /// transcript/src/lib.rs:10-14
    pub fn new() -> Self {
        let mut h: *mut zk_transcript = std::ptr::null_mut();
        let rc = unsafe { zk_transcript_new(&mut h) };
        assert!(rc == 0, "{}", err(rc));
        Self { h }
    }
    /// transcript/src/lib.rs:16-18
    pub fn append(&mut self, new_data: &[u8]) {
        let rc = unsafe { zk_transcript_append(self.h, new_data.as_ptr(), new_data.len()) };
        assert!(rc == 0, "{}", err(rc));
    }
    /// transcript/src/lib.rs:27-30
    pub fn sample_field_element<F: GpuField>(&mut self) -> F {
        let mut out = [F::zero()];
        let rc = unsafe { zk_transcript_sample_field_element(self.h, F::ZK_FIELD, limbs_mut(&mut out)) };
        assert!(rc == 0, "{}", err(rc));
        out[0]
    }
    /// transcript/src/lib.rs:32-34
    pub fn sample_n_field_elements<F: GpuField>(&mut self, n: usize) -> Vec<F> {
        let mut out = vec![F::zero(); n];
        let rc = unsafe { zk_transcript_sample_n_field_elements(self.h, F::ZK_FIELD, n as u64, limbs_mut(&mut out)) };
        assert!(rc == 0, "{}", err(rc));
        out
    }
}

/// sumcheck::SumcheckProof (sumcheck/src/lib.rs:6-11)
#[derive(Debug)]
pub struct SumcheckProof<F: PrimeField> { pub sum: F, pub round_polys: Vec<Vec<F>> }

/// sumcheck::SubClaim (sumcheck/src/lib.rs:17-20): sum = initial_poly(challenges) is the check left to the caller
pub struct SubClaim<F: PrimeField> { pub sum: F, pub challenges: Vec<F> }

/// sumcheck::prover::SumcheckProver (prover.rs:9-12)
pub struct SumcheckProver<const MAX_VAR_DEGREE: u8, F: GpuField> { _marker: PhantomData<F> }

impl<const MAX_VAR_DEGREE: u8, F: GpuField> SumcheckProver<MAX_VAR_DEGREE, F> {
    fn run(poly: ProductPoly<F>, sum: F, absorb: i32) -> Result<(SumcheckProof<F>, Vec<F>), &'static str> {
        let n = poly.n_vars();
        let ns = MAX_VAR_DEGREE as usize + 1;
        let h: Vec<*mut zk_mle> = poly.polynomials.iter().map(|p| p.h).collect();
        let mut rp = vec![F::zero(); n * ns];
        let mut ch = vec![F::zero(); n];
        let s = [sum];
        // the reference takes `poly` by value: the library may use its tables as scratch (consume = 1); they are freed when
        // `poly` drops at the end of this function
        let rc = unsafe { zk_sumcheck_prove(poly.ctx_raw(), h.as_ptr(), h.len() as u64, MAX_VAR_DEGREE as u32, limbs(&s), absorb, 1,
                                            limbs_mut(&mut rp), limbs_mut(&mut ch)) };
        if rc != 0 { return Err(err(rc)); }
        let round_polys = rp.chunks(ns).map(|c| c.to_vec()).collect();
        Ok((SumcheckProof { sum, round_polys }, ch))
    }
    /// prover.rs:15-20
    pub fn prove(poly: ProductPoly<F>, sum: F) -> Result<SumcheckProof<F>, &'static str> { Ok(Self::run(poly, sum, 1)?.0) }
    /// prover.rs:24-30
    pub fn prove_partial(poly: ProductPoly<F>, sum: F) -> Result<(SumcheckProof<F>, Vec<F>), &'static str> {
        Self::run(poly, sum, 0)
    }
    /// `polys.len()` independent `prove_partial` calls (same factor count and arity) proved side by side: one kernel launch per
    /// round for all of them (zk_sumcheck_prove_batch).  Element i equals `prove_partial(polys[i], sums[i])`, bit for bit.
    pub fn prove_partial_batch(polys: Vec<ProductPoly<F>>, sums: Vec<F>) -> Result<Vec<(SumcheckProof<F>, Vec<F>)>, &'static str> {
        if polys.len() != sums.len() { return Err(err(ZK_ERR_BAD_ARG)); }
        if polys.is_empty() { return Ok(Vec::new()); }
        let (b, k, n, ns) = (polys.len(), polys[0].handles().len(), polys[0].n_vars(), MAX_VAR_DEGREE as usize + 1);
        let mut h: Vec<*mut zk_mle> = Vec::with_capacity(b * k);
        for p in &polys {
            let hp = p.handles();
            if hp.len() != k { return Err(err(ZK_ERR_ARITY_MISMATCH)); }
            h.extend(hp.iter().map(|x| *x as *mut zk_mle));
        }
        let (mut rp, mut ch) = (vec![F::zero(); b * n * ns + 1], vec![F::zero(); b * n + 1]);
        let rc = unsafe { zk_sumcheck_prove_batch(polys[0].ctx_raw(), b as u64, h.as_ptr(), k as u64, MAX_VAR_DEGREE as u32, limbs(&sums), 0,
                                                  limbs_mut(&mut rp), limbs_mut(&mut ch)) };
        if rc != 0 { return Err(err(rc)); }
        Ok((0..b).map(|i| (SumcheckProof { sum: sums[i], round_polys: rp[i * n * ns..(i + 1) * n * ns].chunks(ns).map(|c| c.to_vec()).collect() },
                           ch[i * n..(i + 1) * n].to_vec())).collect())
    }
}

/// sumcheck::verifier::SumcheckVerifier (verifier.rs:9-11)
pub struct SumcheckVerifier<F: GpuField> { _marker: PhantomData<F> }

impl<F: GpuField> SumcheckVerifier<F> {
    /// `round_polys` is a `Vec<Vec<F>>` and the reference interpolates every round at its own length (verifier.rs:55-58):
    /// the evaluations go to the library back to back with one length per round.
    fn flatten(proof: &SumcheckProof<F>) -> (Vec<F>, Vec<u32>) {
        let mut lens: Vec<u32> = proof.round_polys.iter().map(|r| r.len() as u32).collect();
        lens.push(0);
        let mut rps: Vec<F> = proof.round_polys.iter().flatten().copied().collect();
        rps.push(F::zero());
        (rps, lens)
    }
    /// verifier.rs:15-33
    pub fn verify(poly: ProductPoly<F>, proof: SumcheckProof<F>) -> Result<bool, &'static str> {
        let (rps, lens) = Self::flatten(&proof);
        let h = poly.handles();
        let s = [proof.sum];
        let mut ok = 0i32;
        let rc = unsafe { zk_sumcheck_verify_lengths(poly.ctx_raw(), h.as_ptr(), h.len() as u64, proof.round_polys.len() as u64,
                                                     lens.as_ptr(), limbs(&s), limbs(&rps), &mut ok) };
        if rc != 0 { return Err(err(rc)); } // "invalid proof: require 1 round poly ..." / "verifier check failed: ..."
        Ok(ok != 0)
    }
    /// verifier.rs:38-41
    pub fn verify_partial(proof: SumcheckProof<F>) -> Result<SubClaim<F>, &'static str> {
        let (rps, lens) = Self::flatten(&proof);
        let n = proof.round_polys.len();
        let s = [proof.sum];
        let mut sum = [F::zero()];
        let mut challenges = vec![F::zero(); n.max(1)];
        let rc = unsafe { zk_sumcheck_verify_partial_lengths(F::ZK_FIELD, n as u64, lens.as_ptr(), limbs(&s), limbs(&rps),
                                                             limbs_mut(&mut sum), limbs_mut(&mut challenges)) };
        if rc != 0 { return Err(err(rc)); }
        challenges.truncate(n);
        Ok(SubClaim { sum: sum[0], challenges })
    }
}

/// fft/src/lib.rs:4-8 (panics like the reference when the length has no root of unity)
pub fn fft<F: GpuField>(coefficients: Vec<F>) -> Vec<F> {
    let c = ctx::<F>().unwrap_or_else(|e| panic!("{}", e));
    let mut out = vec![F::zero(); coefficients.len()];
    let rc = unsafe { zk_fft_host(c.raw, limbs(&coefficients), coefficients.len() as u64, limbs_mut(&mut out)) };
    assert!(rc == 0, "{}", err(rc));
    out
}
/// fft/src/lib.rs:11-19
pub fn ifft<F: GpuField>(evaluations: Vec<F>) -> Vec<F> {
    let c = ctx::<F>().unwrap_or_else(|e| panic!("{}", e));
    let mut out = vec![F::zero(); evaluations.len()];
    let rc = unsafe { zk_ifft_host(c.raw, limbs(&evaluations), evaluations.len() as u64, limbs_mut(&mut out)) };
    assert!(rc == 0, "{}", err(rc));
    out
}
/// fft/src/lib.rs:21-46 — any omega (for a non-primitive one the library uses the literal omega^(i + n/2) form);
/// panics with "values must be a power of 2" like the reference
pub fn fft_internal<F: GpuField>(values: Vec<F>, omega: F) -> Vec<F> {
    let c = ctx::<F>().unwrap_or_else(|e| panic!("{}", e));
    let mut out = vec![F::zero(); values.len()];
    let w = [omega];
    let rc = unsafe { zk_fft_internal_host(c.raw, limbs(&values), values.len() as u64, limbs(&w), limbs_mut(&mut out)) };
    assert!(rc != ZK_ERR_FFT_NOT_POW2 && rc != ZK_ERR_FFT_NO_ROOT, "{}", err(rc));
    assert!(rc == 0, "{}", err(rc));
    out
}

// ---- GKR-shaped driver ---------------------------------------------------------------------------------------------
// The reference has no gkr crate (its building block is prove_partial, prover.rs:24-30; intent at
// evaluation_form.rs:45-48).  These are the bindings of this library's own layered driver.

/// prove_partial on sum_i prod_{f in terms[i]}: (round polys, challenges, every factor at the challenge point)
pub fn prove_partial_terms<const MAX_VAR_DEGREE: u8, F: GpuField>(terms: &[Vec<MultiLinearPolynomial<F>>], sum: F)
    -> Result<(SumcheckProof<F>, Vec<F>, Vec<F>), &'static str> {
    let h: Vec<*mut zk_mle> = terms.iter().flat_map(|t| t.iter().map(|p| p.h)).collect();
    let tk: Vec<u64> = terms.iter().map(|t| t.len() as u64).collect();
    if h.is_empty() { return Err(err(ZK_ERR_EMPTY_PRODUCT)); }
    let first = terms.iter().find(|t| !t.is_empty()).unwrap();
    let n = first[0].n_vars();
    let ns = MAX_VAR_DEGREE as usize + 1;
    let (mut rp, mut ch, mut fin) = (vec![F::zero(); n * ns], vec![F::zero(); n], vec![F::zero(); h.len()]);
    let s = [sum];
    let rc = unsafe { zk_sumcheck_prove_terms(first[0].ctx.raw, h.as_ptr(), tk.as_ptr(), tk.len() as u64, MAX_VAR_DEGREE as u32,
                                              limbs(&s), 0, limbs_mut(&mut rp), limbs_mut(&mut ch), limbs_mut(&mut fin)) };
    if rc != 0 { return Err(err(rc)); }
    Ok((SumcheckProof { sum, round_polys: rp.chunks(ns).map(|c| c.to_vec()).collect() }, ch, fin))
}

/// One layer: 2^log_out gates (op 0 = add, 1 = mul) over the 2^log_in values of the layer below.
pub struct Layer { pub log_out: usize, pub log_in: usize, pub op: Vec<u8>, pub left: Vec<u32>, pub right: Vec<u32> }

pub struct Circuit<F: GpuField> { ctx: Rc<Ctx>, h: *mut zk_circuit, _f: PhantomData<F> }
impl<F: GpuField> Drop for Circuit<F> { fn drop(&mut self) { unsafe { zk_circuit_free(self.h); } } }
impl<F: GpuField> Circuit<F> {
    /// layers[0] = output layer.  Uses the thread's context for `F`, the one every `MultiLinearPolynomial<F>` lives in.
    pub fn new(layers: &[Layer]) -> Result<Self, &'static str> {
        let c = ctx::<F>()?;
        let mut h: *mut zk_circuit = std::ptr::null_mut();
        let rc = unsafe { zk_circuit_create(c.raw, &mut h) };
        if rc != 0 { return Err(err(rc)); }
        let circuit = Circuit { ctx: c, h, _f: PhantomData };
        for l in layers {
            let gates = 1usize << l.log_out;
            if l.op.len() != gates || l.left.len() != gates || l.right.len() != gates { return Err(err(-20)); }
            let rc = unsafe { zk_circuit_add_layer(h, l.log_out as u64, l.log_in as u64, l.op.as_ptr(), l.left.as_ptr(), l.right.as_ptr()) };
            if rc != 0 { return Err(err(rc)); }
        }
        Ok(circuit)
    }
    fn proof_elems(&self) -> usize {
        let mut n = 0u64;
        unsafe { zk_circuit_proof_elems(self.h, &mut n); }
        n as usize
    }
    /// -> (outputs, proof elements: per layer [round polys #1 | round polys #2 | W(u) | W(v)])
    pub fn prove(&self, input: &MultiLinearPolynomial<F>, seed: &[u8; 32]) -> Result<(MultiLinearPolynomial<F>, Vec<F>), &'static str> {
        let mut proof = vec![F::zero(); self.proof_elems()];
        let mut out: *mut zk_mle = std::ptr::null_mut();
        let rc = unsafe { zk_gkr_prove(self.h, input.h, seed.as_ptr(), &mut out, limbs_mut(&mut proof)) };
        if rc != 0 { return Err(err(rc)); }
        Ok((MultiLinearPolynomial::from_handle(Rc::clone(&self.ctx), out), proof))
    }
    /// Ok(true) accept / Ok(false) reject (a sumcheck round check, a layer's wiring check or the input check failed)
    pub fn verify(&self, input: &MultiLinearPolynomial<F>, outputs: &MultiLinearPolynomial<F>, seed: &[u8; 32], proof: &[F])
        -> Result<bool, &'static str> {
        if proof.len() != self.proof_elems() { return Ok(false); } // the library reads exactly proof_elems elements
        match unsafe { zk_gkr_verify(self.h, input.h, outputs.h, seed.as_ptr(), limbs(proof)) } {
            0 => Ok(true),
            ZK_ERR_VERIFY_SUM | ZK_ERR_GKR_REJECT => Ok(false),
            rc => Err(err(rc)),
        }
    }
}
