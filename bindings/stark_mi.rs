//! stark_mi.rs -- the Rust side of the drop-in boundary: raw declarations of every entry point of
//! `include/stark_mi.h` (libstarkmi.so, hand-written HIP for gfx950 behind a C ABI) and thin safe wrappers for
//! the methods of 0xSooki/stark-rs that stand in front of it.  Add to the reference as `src/mi.rs`
//! (`mod mi;`) with the `build.rs` of INTEGRATION.md; the reference itself has no FFI and no dependencies,
//! so this file uses `std` only.
//!
//! What each wrapper replaces (reference file:line):
//!   interpolate_domain  src/univariate/interpolate.rs:6-44     eval_domain   src/univariate/eval.rs:16-21
//!   scale               src/univariate/mod.rs:99-113           mul / div     src/univariate/mul.rs:6-29, div.rs:6-52
//!   hash_leaves         src/hash.rs:32-35 via src/fri.rs:118-121   combine_pairs  src/hash.rs:41-46
//!   MerkleTree          src/merkle.rs:11-80                    fold_codeword src/fri.rs:57-91
//!   fri_prove           src/fri.rs:250-311                     fri_verify    src/fri.rs:313-504
//!   lde / trace_pack    src/trace.rs:21-34 + per-column interpolate / evaluate (no reference function)
//!
//! Values cross the boundary as the reference's wire format: field elements as little-endian u64
//! (`FieldElement::value`, src/stream.rs:45), digests as 32 raw bytes (`Hash.0`).  A non-zero status becomes
//! the reference's own panic message (`check`), so `#[should_panic(expected = "...")]` tests keep passing.
//!
//! The image this was written in has no rustc: tests/test_rust_binding.py checks every declaration below
//! against the header (symbol set, arity, pointer depth and constness, integer widths, struct layouts).
#![allow(non_camel_case_types, dead_code, clippy::too_many_arguments, clippy::missing_safety_doc)]

use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

// BEGIN GENERATED (tools/gen_rust_bindings.py from include/stark_mi.h) -- do not edit by hand
/// Status codes (include/stark_mi.h): 0 = ok; -1..-18 mirror a reference panic; the rest are contract or runtime errors.
pub const SMI_OK: c_int = 0;
pub const SMI_ERR_NO_INVERSE: c_int = -1;
pub const SMI_ERR_DIV_BY_ZERO: c_int = -2;
pub const SMI_ERR_NOT_POW2: c_int = -3;
pub const SMI_ERR_ROOT_TOO_LARGE: c_int = -4;
pub const SMI_ERR_EMPTY_LEAVES: c_int = -5;
pub const SMI_ERR_LEAVES_NOT_POW2: c_int = -6;
pub const SMI_ERR_INDEX_OOB: c_int = -7;
pub const SMI_ERR_DOMAIN_NOT_POW2: c_int = -8;
pub const SMI_ERR_EXPANSION_NOT_POW2: c_int = -9;
pub const SMI_ERR_EXPANSION_TOO_SMALL: c_int = -10;
pub const SMI_ERR_CODEWORD_LEN: c_int = -11;
pub const SMI_ERR_SAMPLE_ENTROPY: c_int = -12;
pub const SMI_ERR_SAMPLE_TOO_MANY: c_int = -13;
pub const SMI_ERR_LEN_MISMATCH: c_int = -14;
pub const SMI_ERR_EMPTY_DOMAIN: c_int = -15;
pub const SMI_ERR_WRONG_FIELD: c_int = -16;
pub const SMI_ERR_POLY_DIV_BY_ZERO: c_int = -18;
pub const SMI_ERR_NO_ROUNDS: c_int = -17;
pub const SMI_ERR_BAD_ARG: c_int = -50;
pub const SMI_ERR_NON_CANONICAL: c_int = -51;
pub const SMI_ERR_UNSUPPORTED_PRIME: c_int = -52;
pub const SMI_ERR_NOT_GEOMETRIC: c_int = -53;
pub const SMI_ERR_COLUMNS_NOT_BOUND: c_int = -54;
pub const SMI_ERR_GRIND_EXHAUSTED: c_int = -55;
pub const SMI_ERR_LOOKUP_MISSING: c_int = -56;
pub const SMI_ERR_HIP: c_int = -100;
pub const SMI_ERR_NO_DEVICE: c_int = -101;
pub const SMI_ERR_OOM: c_int = -102;
pub const SMI_ERR_RCCL: c_int = -103;
pub const SMI_MGPU_ID_BYTES: usize = 128;

#[repr(C)] pub struct smi_ctx { _p: [u8; 0] }
#[repr(C)] pub struct smi_tree { _p: [u8; 0] }
#[repr(C)] pub struct smi_fri_run { _p: [u8; 0] }
#[repr(C)] pub struct smi_mgpu { _p: [u8; 0] }

#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct smi_kernel_time {
    pub name: [c_char; 56],
    pub launches: u32,
    pub total_ms: f64,
    pub alg_bytes: f64,
    pub alg_mixes: f64,
}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct smi_fri_cfg {
    pub omega: u64,
    pub offset: u64,
    pub domain_length: u64,
    pub expansion_factor: u64,
    pub num_colinearity_tests: u64,
}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct smi_stark_cfg {
    pub log_n: u32,
    pub log_blowup: u32,
    pub n_cols: u32,
    pub row_leaves: u32,
    pub trace_offset: u64,
    pub lde_offset: u64,
    pub num_colinearity_tests: u64,
    pub open_columns: u64,
}

/// smi_mgpu_coll: three caller-supplied collectives (device pointers; 0 = ok), how another transport is plugged in
#[repr(C)] #[derive(Clone, Copy)]
pub struct smi_mgpu_coll {
    pub user: *mut c_void,
    pub all_gather: Option<unsafe extern "C" fn(user: *mut c_void, d_send: *const c_void, d_recv: *mut c_void, bytes_per_rank: usize) -> c_int>,
    pub exchange: Option<unsafe extern "C" fn(user: *mut c_void, n_send: c_int, send_peer: *const c_int, d_send: *const *mut c_void, send_bytes: *const usize,
                                                n_recv: c_int, recv_peer: *const c_int, d_recv: *const *mut c_void, recv_bytes: *const usize) -> c_int>,
    pub all_reduce_sum_u8: Option<unsafe extern "C" fn(user: *mut c_void, d_buf: *mut c_void, bytes: usize) -> c_int>,
}

/// smi_air: the flat tables of an AIR (host pointers; the entry points take it as `*const c_void`)
#[repr(C)] #[derive(Clone, Copy)]
pub struct smi_air {
    pub n_constraints: u32,
    pub n_terms: u32,
    pub n_factors: u32,
    pub n_boundary: u32,
    pub constraint_first_term: *const u32,
    pub term_coeff: *const u64,
    pub term_first_factor: *const u32,
    pub factor_var: *const u32,
    pub factor_exp: *const u32,
    pub boundary_col: *const u32,
    pub boundary_row: *const u64,
    pub boundary_value: *const u64,
    pub n_periodic: u32,
    pub window: u32,
    pub periodic_log_period: *const u32,
    pub periodic_value: *const u64,
}
/// smi_air_perm: one permutation argument (host pointers; the entry points take it as `*const c_void`)
#[repr(C)] #[derive(Clone, Copy)]
pub struct smi_air_perm {
    pub width: u32,
    pub reserved0: u32,
    pub left_col: *const u32,
    pub right_col: *const u32,
}
/// smi_air_lookup: one lookup argument (host pointers; the entry points take it as `*const c_void`)
#[repr(C)] #[derive(Clone, Copy)]
pub struct smi_air_lookup {
    pub width: u32,
    pub mult_col: u32,
    pub lookup_col: *const u32,
    pub table_col: *const u32,
}
/// smi_air_arg: one argument of an argument list (host pointers; the entry points take the list as `*const c_void`)
#[repr(C)] #[derive(Clone, Copy)]
pub struct smi_air_arg {
    pub kind: u32,
    pub width: u32,
    pub mult_col: u32,
    pub reserved0: u32,
    pub a_col: *const u32,
    pub b_col: *const u32,
}
/// smi_air_args: an argument list (host pointers; the entry points take the list as `*const c_void`)
#[repr(C)] #[derive(Clone, Copy)]
pub struct smi_air_args {
    pub count: u32,
    pub reserved0: u32,
    pub arg: *const smi_air_arg,
}
/// smi_air_xarg: one argument of a list with selectors and periodic members (host pointers; the entry points take the list as `*const c_void`)
#[repr(C)] #[derive(Clone, Copy)]
pub struct smi_air_xarg {
    pub kind: u32,
    pub width: u32,
    pub mult_col: u32,
    pub reserved0: u32,
    pub a_var: *const u32,
    pub b_var: *const u32,
    pub a_sel: u32,
    pub b_sel: u32,
}
/// smi_air_xargs: an argument list with selectors and periodic members (host pointers; the entry points take the list as `*const c_void`)
#[repr(C)] #[derive(Clone, Copy)]
pub struct smi_air_xargs {
    pub count: u32,
    pub reserved0: u32,
    pub arg: *const smi_air_xarg,
}
pub const SMI_AIR_MAX_CONSTRAINTS: u32 = 64;
pub const SMI_AIR_MAX_TERMS: u32 = 1024;
pub const SMI_AIR_MAX_TERM_FACTORS: u32 = 8;
pub const SMI_AIR_MAX_EXP: u32 = 255;
pub const SMI_AIR_MAX_BOUNDARY_PER_COL: u32 = 16;
pub const SMI_AIR_MAX_PERIODIC: u32 = 16;
pub const SMI_AIR_MAX_WINDOW: u32 = 4;
pub const SMI_GRIND_MAX_BITS: u32 = 32;
pub const SMI_PERM_MAX_WIDTH: u32 = 8;
pub const SMI_LOOKUP_MAX_WIDTH: u32 = 8;
pub const SMI_ARGS_MAX: u32 = 8;
pub const SMI_ARG_PERM: u32 = 0;
pub const SMI_ARG_LOOKUP: u32 = 1;
pub const SMI_ARG_NO_SELECTOR: u32 = 0xffffffff;
pub const SMI_ARG_NEXT_ROW: u32 = 0x40000000;
pub const SMI_ARG_MAX_TUPLES: u32 = 4;
pub const SMI_ARG_TUPLES_SHIFT: u32 = 8;

#[link(name = "starkmi")]
extern "C" {
    pub fn smi_status_string(status: c_int) -> *const c_char;
    pub fn smi_last_error(ctx: *const smi_ctx) -> *const c_char;
    pub fn smi_version() -> *const c_char;
    pub fn smi_ctx_create(p: u64, g: u64, device: c_int, out: *mut *mut smi_ctx) -> c_int;
    pub fn smi_ctx_destroy(ctx: *mut smi_ctx);
    pub fn smi_ctx_set_stream(ctx: *mut smi_ctx, hip_stream: *mut c_void) -> c_int;
    pub fn smi_ctx_sync(ctx: *mut smi_ctx) -> c_int;
    pub fn smi_ctx_profile(ctx: *mut smi_ctx, enable: c_int) -> c_int;
    pub fn smi_ctx_profile_read(ctx: *mut smi_ctx, out: *mut smi_kernel_time, cap: usize, n: *mut usize) -> c_int;
    pub fn smi_ctx_profile_only(ctx: *mut smi_ctx, name_part: *const c_char) -> c_int;
    pub fn smi_ctx_copy_probe(ctx: *mut smi_ctx, enable: c_int) -> c_int;
    pub fn smi_ctx_mix_probe(ctx: *mut smi_ctx, mixes: u32, mixes_per_s: *mut f64) -> c_int;
    pub fn smi_ctx_lde_two_pass(ctx: *mut smi_ctx, enable: c_int) -> c_int;
    pub fn smi_ctx_modulus(ctx: *const smi_ctx) -> u64;
    pub fn smi_ctx_two_adicity(ctx: *const smi_ctx) -> u32;
    pub fn smi_prim_nth_root(ctx: *const smi_ctx, n: u64, out: *mut u64) -> c_int;
    pub fn smi_ff_inv(ctx: *const smi_ctx, x: u64, out: *mut u64) -> c_int;
    pub fn smi_ff_exp(ctx: *const smi_ctx, base: u64, e: u64, out: *mut u64) -> c_int;
    pub fn smi_ff_mul(ctx: *const smi_ctx, a: u64, b: u64, out: *mut u64) -> c_int;
    pub fn smi_intt(ctx: *mut smi_ctx, values: *const u64, coeffs: *mut u64, log_n: u32, offset: u64) -> c_int;
    pub fn smi_coset_ntt(ctx: *mut smi_ctx, coeffs: *const u64, n_coeffs: usize, evals: *mut u64, log_N: u32, offset: u64) -> c_int;
    pub fn smi_poly_scale(ctx: *mut smi_ctx, coeffs: *const u64, n: usize, factor: u64, out: *mut u64) -> c_int;
    pub fn smi_poly_mul(ctx: *mut smi_ctx, a: *const u64, na: usize, b: *const u64, nb: usize, out: *mut u64, n_out: *mut usize) -> c_int;
    pub fn smi_poly_div(ctx: *mut smi_ctx, a: *const u64, na: usize, b: *const u64, nb: usize, q: *mut u64, nq: *mut usize, r: *mut u64, nr: *mut usize) -> c_int;
    pub fn smi_domain_is_geometric(ctx: *const smi_ctx, domain: *const u64, n: usize, offset: *mut u64) -> c_int;
    pub fn smi_poly_zerofier(ctx: *mut smi_ctx, domain: *const u64, n: usize, coeffs: *mut u64) -> c_int;
    pub fn smi_poly_eval_points(ctx: *mut smi_ctx, coeffs: *const u64, n_coeffs: usize, points: *const u64, n_points: usize, values: *mut u64) -> c_int;
    pub fn smi_poly_interpolate_points(ctx: *mut smi_ctx, domain: *const u64, values: *const u64, n: usize, coeffs: *mut u64) -> c_int;
    pub fn smi_lde(ctx: *mut smi_ctx, cols: *const u64, n_cols: u32, log_n: u32, log_blowup: u32, trace_offset: u64, lde_offset: u64, out: *mut u64) -> c_int;
    pub fn smi_trace_pack(ctx: *const smi_ctx, rows_i128: *const c_void, n_rows: usize, n_cols: usize, cols_out: *mut u64) -> c_int;
    pub fn smi_hash_leaves(ctx: *mut smi_ctx, elems: *const u64, n: usize, digests: *mut u8) -> c_int;
    pub fn smi_hash_combine_pairs(ctx: *mut smi_ctx, digests: *const u8, n_pairs: usize, out: *mut u8) -> c_int;
    pub fn smi_hash_bytes(ctx: *mut smi_ctx, msg: *const u8, len: usize, out: *mut u8) -> c_int;
    pub fn smi_hash_bytes_batch(ctx: *mut smi_ctx, msgs: *const u8, n: usize, msg_len: usize, out: *mut u8) -> c_int;
    pub fn smi_merkle_commit(ctx: *mut smi_ctx, leaves: *const u8, n: usize, root: *mut u8) -> c_int;
    pub fn smi_merkle_new(ctx: *mut smi_ctx, leaves: *const u8, n: usize, out: *mut *mut smi_tree) -> c_int;
    pub fn smi_merkle_from_codeword(ctx: *mut smi_ctx, codeword: *const u64, n: usize, out: *mut *mut smi_tree) -> c_int;
    pub fn smi_merkle_root(ctx: *mut smi_ctx, t: *const smi_tree, root: *mut u8) -> c_int;
    pub fn smi_merkle_open(ctx: *mut smi_ctx, t: *const smi_tree, index: usize, path: *mut u8, depth: *mut usize) -> c_int;
    pub fn smi_merkle_level(ctx: *mut smi_ctx, t: *const smi_tree, level: u32, out: *mut u8, n_out: *mut usize) -> c_int;
    pub fn smi_merkle_verify_batch(ctx: *mut smi_ctx, leaves: *const u8, indices: *const u64, paths: *const u8, k: usize, depth: usize, root: *const u8, ok: *mut u8) -> c_int;
    pub fn smi_merkle_num_leaves(t: *const smi_tree) -> usize;
    pub fn smi_merkle_free(t: *mut smi_tree);
    pub fn smi_fri_check(ctx: *const smi_ctx, cfg: *const smi_fri_cfg) -> c_int;
    pub fn smi_fri_num_rounds(cfg: *const smi_fri_cfg, rounds: *mut u64) -> c_int;
    pub fn smi_fri_fold(ctx: *mut smi_ctx, codeword: *const u64, len: usize, alpha: u64, offset: u64, omega: u64, out: *mut u64) -> c_int;
    pub fn smi_fri_commit(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, codeword: *const u64, len: usize, roots: *mut u8, alphas: *mut u64, last_codeword: *mut u64, last_len: *mut usize, run: *mut *mut smi_fri_run) -> c_int;
    pub fn smi_fri_commit_fs(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, codeword: *const u64, len: usize, roots: *mut u8, alphas: *mut u64, last_codeword: *mut u64, last_len: *mut usize, run: *mut *mut smi_fri_run) -> c_int;
    pub fn smi_fri_prove(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, codeword: *const u64, len: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64) -> c_int;
    pub fn smi_fri_prove_fs(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, codeword: *const u64, len: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64) -> c_int;
    pub fn smi_fri_verify(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, proof: *const u8, proof_len: usize, accept: *mut c_int, pv_indices: *mut u64, pv_values: *mut u64, n_pv: *mut usize) -> c_int;
    pub fn smi_fri_verify_fs(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, proof: *const u8, proof_len: usize, accept: *mut c_int, pv_indices: *mut u64, pv_values: *mut u64, n_pv: *mut usize, consumed: *mut usize) -> c_int;
    pub fn smi_fri_run_num_codewords(run: *const smi_fri_run, n: *mut usize) -> c_int;
    pub fn smi_fri_run_codeword(run: *mut smi_fri_run, round: usize, out: *mut u64, len: *mut usize) -> c_int;
    pub fn smi_fri_run_open(run: *mut smi_fri_run, round: usize, index: usize, path: *mut u8, depth: *mut usize) -> c_int;
    pub fn smi_fri_run_free(run: *mut smi_fri_run);
    pub fn smi_free(p: *mut c_void);
    pub fn smi_dev_alloc(ctx: *mut smi_ctx, bytes: usize, d_ptr: *mut *mut c_void) -> c_int;
    pub fn smi_dev_free(ctx: *mut smi_ctx, d_ptr: *mut c_void) -> c_int;
    pub fn smi_dev_upload_u64(ctx: *mut smi_ctx, host: *const u64, n: usize, d_out: *mut u32, reduce: c_int) -> c_int;
    pub fn smi_dev_download_u64(ctx: *mut smi_ctx, d_in: *const u32, n: usize, host: *mut u64) -> c_int;
    pub fn smi_dev_ntt(ctx: *mut smi_ctx, d_in: *const u32, d_out: *mut u32, log_n: u32, n_in: usize, batch: u32, in_stride: usize, out_stride: usize, inverse: c_int, offset: u64, post_scale: u64) -> c_int;
    pub fn smi_dev_lde(ctx: *mut smi_ctx, d_cols: *const u32, n_cols: u32, log_n: u32, log_blowup: u32, trace_offset: u64, lde_offset: u64, d_out: *mut u32) -> c_int;
    pub fn smi_dev_hash_leaves(ctx: *mut smi_ctx, d_elems: *const u32, n: usize, d_digests: *mut u8) -> c_int;
    pub fn smi_dev_merkle_build(ctx: *mut smi_ctx, d_elems: *const u32, n: usize, d_nodes: *mut u8) -> c_int;
    pub fn smi_dev_merkle_build_rows(ctx: *mut smi_ctx, d_cols: *const u32, n_cols: u32, col_stride: usize, n: usize, d_nodes: *mut u8) -> c_int;
    pub fn smi_dev_merkle_build_cosets(ctx: *mut smi_ctx, d_cols: *const u32, n_cols: u32, col_stride: usize, n: usize, d_nodes: *mut u8) -> c_int;
    pub fn smi_dev_merkle_from_digests(ctx: *mut smi_ctx, n: usize, d_nodes: *mut u8) -> c_int;
    pub fn smi_dev_hash_bytes(ctx: *mut smi_ctx, d_msg: *const u8, len: usize, d_out32: *mut u8) -> c_int;
    pub fn smi_dev_fri_fold(ctx: *mut smi_ctx, d_in: *const u32, len: usize, d_alpha: *const u64, offset: u64, omega: u64, d_out: *mut u32) -> c_int;
    pub fn smi_dev_fri_fold_shard(ctx: *mut smi_ctx, d_lo: *const u32, d_hi: *const u32, count: usize, index0: usize, full_len: usize, d_alpha: *const u64, offset: u64, omega: u64, d_out: *mut u32) -> c_int;
    pub fn smi_dev_fri_prove(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, d_codeword: *const u32, len: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, run: *mut *mut smi_fri_run) -> c_int;
    pub fn smi_dev_fri_prove_fs(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, d_codeword: *const u32, len: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, run: *mut *mut smi_fri_run) -> c_int;
    pub fn smi_dev_combine_columns(ctx: *mut smi_ctx, d_cols: *const u32, n_cols: u32, len: usize, stride: usize, d_weights: *const u64, d_out: *mut u32) -> c_int;
    pub fn smi_dev_stark_prove(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, d_trace_cols: *const u32, column_roots: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64) -> c_int;
    pub fn smi_stark_verify(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, column_roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int) -> c_int;
    pub fn smi_air_plan(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, degree: *mut u32, fri_expansion: *mut u64) -> c_int;
    pub fn smi_air_last_error() -> *const c_char;
    pub fn smi_dev_air_compose(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_lde: *const u32, stride: usize, d_weights: *const u64, d_out: *mut u32) -> c_int;
    pub fn smi_dev_air_check(ctx: *mut smi_ctx, air: *const c_void, n_cols: u32, log_n: u32, d_trace_cols: *const u32, ok: *mut c_int, constraint: *mut u32, row: *mut u64) -> c_int;
    pub fn smi_dev_air_prove(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_trace_cols: *const u32, column_roots: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64) -> c_int;
    pub fn smi_air_verify(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, column_roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int) -> c_int;
    pub fn smi_dev_air_prove_rows(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_trace_cols: *const u32, row_root: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64) -> c_int;
    pub fn smi_air_verify_rows(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, row_root: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int) -> c_int;
    pub fn smi_ext_mul(p: u64, g: u64, a: *const u64, b: *const u64, out: *mut u64) -> c_int;
    pub fn smi_ext_inv(p: u64, g: u64, a: *const u64, out: *mut u64) -> c_int;
    pub fn smi_dev_fri_fold_ext(ctx: *mut smi_ctx, d_in: *const u32, len: usize, stride: usize, d_alpha: *const u64, offset: u64, omega: u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_air_compose_ext(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_lde: *const u32, stride: usize, d_weights: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_fri_prove_ext(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, d_codeword: *const u32, len: usize, stride: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64) -> c_int;
    pub fn smi_fri_verify_ext(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, proof: *const u8, proof_len: usize, accept: *mut c_int, pv_indices: *mut u64, pv_values: *mut u64, n_pv: *mut usize, consumed: *mut usize) -> c_int;
    pub fn smi_dev_air_prove_ext(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_trace_cols: *const u32, row_root: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64) -> c_int;
    pub fn smi_air_verify_ext(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, row_root: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int) -> c_int;
    pub fn smi_grind_check(transcript: *const u8, transcript_len: usize, nonce: u64, bits: u32, ok: *mut c_int) -> c_int;
    pub fn smi_dev_grind(ctx: *mut smi_ctx, transcript: *const u8, transcript_len: usize, bits: u32, max_tries: u64, nonce: *mut u64) -> c_int;
    pub fn smi_dev_fri_prove_ext_pow(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, d_codeword: *const u32, len: usize, stride: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, grind_bits: u32, nonce: *mut u64) -> c_int;
    pub fn smi_fri_verify_ext_pow(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, proof: *const u8, proof_len: usize, accept: *mut c_int, pv_indices: *mut u64, pv_values: *mut u64, n_pv: *mut usize, consumed: *mut usize, grind_bits: u32) -> c_int;
    pub fn smi_dev_air_prove_ext_pow(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_trace_cols: *const u32, row_root: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32) -> c_int;
    pub fn smi_air_verify_ext_pow(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, row_root: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_fri_fold4_layout(cfg: *const smi_fri_cfg, folds: *mut u64, last_len: *mut u64, proof_len: *mut usize) -> c_int;
    pub fn smi_dev_fri_fold4_ext(ctx: *mut smi_ctx, d_in: *const u32, len: usize, stride: usize, d_alpha: *const u64, offset: u64, omega: u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_fri_prove_ext_fold4(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, d_codeword: *const u32, len: usize, stride: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, grind_bits: u32, nonce: *mut u64) -> c_int;
    pub fn smi_fri_verify_ext_fold4(ctx: *mut smi_ctx, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, proof: *const u8, proof_len: usize, accept: *mut c_int, pv_indices: *mut u64, pv_values: *mut u64, n_pv: *mut usize, consumed: *mut usize, grind_bits: u32) -> c_int;
    pub fn smi_dev_air_prove_ext_fold4(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_trace_cols: *const u32, row_root: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32) -> c_int;
    pub fn smi_air_verify_ext_fold4(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, row_root: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_plan_perm(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, perm: *const c_void, degree: *mut u32, fri_expansion: *mut u64) -> c_int;
    pub fn smi_dev_perm_column(ctx: *mut smi_ctx, perm: *const c_void, d_trace_cols: *const u32, n_cols: u32, log_n: u32, challenges: *const u64, d_z: *mut u32, z_stride: usize, closes: *mut c_int) -> c_int;
    pub fn smi_dev_air_compose_perm(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, perm: *const c_void, d_lde: *const u32, stride: usize, d_z_lde: *const u32, z_stride: usize, challenges: *const u64, d_weights: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_air_prove_perm(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, perm: *const c_void, d_trace_cols: *const u32, roots: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32, closes: *mut c_int) -> c_int;
    pub fn smi_air_verify_perm(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, perm: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_plan_lookup(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, lookup: *const c_void, degree: *mut u32, fri_expansion: *mut u64) -> c_int;
    pub fn smi_dev_lookup_multiplicities(ctx: *mut smi_ctx, lookup: *const c_void, d_trace_cols: *const u32, n_cols: u32, log_n: u32, d_mult: *mut u32) -> c_int;
    pub fn smi_dev_lookup_column(ctx: *mut smi_ctx, lookup: *const c_void, d_trace_cols: *const u32, n_cols: u32, log_n: u32, challenges: *const u64, d_s: *mut u32, s_stride: usize, closes: *mut c_int) -> c_int;
    pub fn smi_dev_air_compose_lookup(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, lookup: *const c_void, d_lde: *const u32, stride: usize, d_s_lde: *const u32, s_stride: usize, challenges: *const u64, d_weights: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_air_prove_lookup(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, lookup: *const c_void, d_trace_cols: *const u32, roots: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32, closes: *mut c_int) -> c_int;
    pub fn smi_air_verify_lookup(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, lookup: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_plan_args(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, args: *const c_void, degree: *mut u32, fri_expansion: *mut u64) -> c_int;
    pub fn smi_dev_args_columns(ctx: *mut smi_ctx, args: *const c_void, d_trace_cols: *const u32, n_cols: u32, log_n: u32, challenges: *const u64, d_c: *mut u32, c_stride: usize, closes: *mut u32) -> c_int;
    pub fn smi_dev_air_compose_args(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, args: *const c_void, d_lde: *const u32, stride: usize, d_c_lde: *const u32, c_stride: usize, challenges: *const u64, d_weights: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_air_prove_args(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, args: *const c_void, d_trace_cols: *const u32, roots: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32, closes: *mut u32) -> c_int;
    pub fn smi_air_verify_args(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, args: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_plan_xargs(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, degree: *mut u32, fri_expansion: *mut u64) -> c_int;
    pub fn smi_dev_xargs_multiplicities(ctx: *mut smi_ctx, air: *const c_void, xargs: *const c_void, a: u32, d_trace_cols: *const u32, n_cols: u32, log_n: u32, d_mult: *mut u32) -> c_int;
    pub fn smi_dev_xargs_columns(ctx: *mut smi_ctx, air: *const c_void, xargs: *const c_void, d_trace_cols: *const u32, n_cols: u32, log_n: u32, challenges: *const u64, d_c: *mut u32, c_stride: usize, closes: *mut u32) -> c_int;
    pub fn smi_dev_air_compose_xargs(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, d_lde: *const u32, stride: usize, d_c_lde: *const u32, c_stride: usize, challenges: *const u64, d_weights: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_air_prove_xargs(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, d_trace_cols: *const u32, roots: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32, closes: *mut u32) -> c_int;
    pub fn smi_air_verify_xargs(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_plan_deep(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, degree: *mut u32, segments: *mut u32) -> c_int;
    pub fn smi_air_deep_layout(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, proof_len: *mut usize) -> c_int;
    pub fn smi_dev_poly_eval_ext(ctx: *mut smi_ctx, d_coeffs: *const u32, n_cols: u32, n_coeffs: usize, stride: usize, points: *const u64, n_points: u32, out: *mut u64) -> c_int;
    pub fn smi_dev_deep_compose(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, n_segments: u32, d_lde: *const u32, stride: usize, d_seg: *const u32, seg_stride: usize, z: *const u64, ood: *const u64, challenges: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_poly_eval_ext_shifts(ctx: *mut smi_ctx, d_coeffs: *const u32, n_cols: u32, n_coeffs: usize, stride: usize, z: *const u64, w: u64, n_shifts: u32, out: *mut u64) -> c_int;
    pub fn smi_dev_deep_compose_window(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, window: u32, n_segments: u32, d_lde: *const u32, stride: usize, d_seg: *const u32, seg_stride: usize, z: *const u64, ood: *const u64, challenges: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_air_prove_deep(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_trace_cols: *const u32, roots: *mut u8, ood: *mut u64, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32) -> c_int;
    pub fn smi_air_verify_deep(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_plan_deep_xargs(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, degree: *mut u32, segments: *mut u32) -> c_int;
    pub fn smi_air_deep_xargs_layout(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, proof_len: *mut usize) -> c_int;
    pub fn smi_dev_deep_compose_args(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, n_args: u32, n_segments: u32, d_lde: *const u32, stride: usize, d_c_lde: *const u32, c_stride: usize, d_seg: *const u32, seg_stride: usize, z: *const u64, ood: *const u64, challenges: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_air_prove_deep_xargs(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, d_trace_cols: *const u32, roots: *mut u8, ood: *mut u64, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32, closes: *mut u32) -> c_int;
    pub fn smi_air_verify_deep_xargs(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_deep_fold4_layout(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, folds: *mut u64, proof_len: *mut usize) -> c_int;
    pub fn smi_dev_air_prove_deep_fold4(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_trace_cols: *const u32, roots: *mut u8, ood: *mut u64, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32) -> c_int;
    pub fn smi_air_verify_deep_fold4(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_deep_xargs_fold4_layout(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, folds: *mut u64, proof_len: *mut usize) -> c_int;
    pub fn smi_dev_air_prove_deep_xargs_fold4(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, d_trace_cols: *const u32, roots: *mut u8, ood: *mut u64, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32, closes: *mut u32) -> c_int;
    pub fn smi_air_verify_deep_xargs_fold4(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_plan_deep_zk(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, degree: *mut u32, segments: *mut u32, k_t: *mut u32, k_s: *mut u32) -> c_int;
    pub fn smi_dev_random_fill(ctx: *mut smi_ctx, seed: *const u8, stream_id: u64, d_out: *mut u32, count: usize) -> c_int;
    pub fn smi_dev_zk_segments(ctx: *mut smi_ctx, d_h: *const u32, h_stride: usize, h_len: usize, log_n: u32, k_s: u32, n_segments: u32, d_rho: *const u32, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_air_deep_zk_layout(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, folds: *mut u64, proof_len: *mut usize) -> c_int;
    pub fn smi_dev_air_prove_deep_zk(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, d_trace_cols: *mut u32, seed: *const u8, roots: *mut u8, ood: *mut u64, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32) -> c_int;
    pub fn smi_air_verify_deep_zk(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_air_plan_deep_zk_xargs(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, degree: *mut u32, segments: *mut u32, k_t: *mut u32, k_s: *mut u32) -> c_int;
    pub fn smi_air_deep_zk_xargs_layout(p: u64, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, folds: *mut u64, proof_len: *mut usize) -> c_int;
    pub fn smi_dev_xargs_multiplicities_rows(ctx: *mut smi_ctx, air: *const c_void, xargs: *const c_void, a: u32, d_trace_cols: *const u32, n_cols: u32, log_n: u32, rows: usize, d_mult: *mut u32) -> c_int;
    pub fn smi_dev_zk_args_tail(ctx: *mut smi_ctx, d_c: *mut u32, c_stride: usize, log_n: u32, k_t: u32, n_args: u32, d_rnd: *const u32, closing: *mut u64) -> c_int;
    pub fn smi_dev_air_compose_zk_xargs(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, d_lde: *const u32, stride: usize, d_c_lde: *const u32, c_stride: usize, challenges: *const u64, d_weights: *const u64, d_out: *mut u32, out_stride: usize) -> c_int;
    pub fn smi_dev_air_prove_deep_zk_xargs(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, d_trace_cols: *mut u32, seed: *const u8, roots: *mut u8, ood: *mut u64, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64, stage_ms: *mut f64, grind_bits: u32, closes: *mut u32) -> c_int;
    pub fn smi_air_verify_deep_zk_xargs(ctx: *mut smi_ctx, cfg: *const smi_stark_cfg, air: *const c_void, xargs: *const c_void, roots: *const u8, proof: *const u8, proof_len: usize, accept: *mut c_int, grind_bits: u32) -> c_int;
    pub fn smi_mgpu_unique_id(id: *mut u8) -> c_int;
    pub fn smi_mgpu_create(ctx: *mut smi_ctx, id: *const u8, rank: c_int, world: c_int, out: *mut *mut smi_mgpu) -> c_int;
    pub fn smi_mgpu_create_with(ctx: *mut smi_ctx, ops: *const smi_mgpu_coll, rank: c_int, world: c_int, out: *mut *mut smi_mgpu) -> c_int;
    pub fn smi_mgpu_destroy(m: *mut smi_mgpu);
    pub fn smi_mgpu_set_min_block(m: *mut smi_mgpu, min_block: usize) -> c_int;
    pub fn smi_mgpu_fri_commit(m: *mut smi_mgpu, cfg: *const smi_fri_cfg, d_block: *const u32, block_len: usize, roots: *mut u8, alphas: *mut u64, last_codeword: *mut u64, last_len: *mut usize) -> c_int;
    pub fn smi_mgpu_fri_prove(m: *mut smi_mgpu, cfg: *const smi_fri_cfg, d_block: *const u32, block_len: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64) -> c_int;
    pub fn smi_mgpu_fri_commit_fs(m: *mut smi_mgpu, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, d_block: *const u32, block_len: usize, roots: *mut u8, alphas: *mut u64, last_codeword: *mut u64, last_len: *mut usize) -> c_int;
    pub fn smi_mgpu_fri_prove_fs(m: *mut smi_mgpu, cfg: *const smi_fri_cfg, transcript: *const u8, transcript_len: usize, d_block: *const u32, block_len: usize, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64) -> c_int;
    pub fn smi_mgpu_lde(m: *mut smi_mgpu, d_trace_cols: *const u32, n_cols: u32, log_n: u32, log_blowup: u32, trace_offset: u64, lde_offset: u64, d_out_blocks: *mut u32) -> c_int;
    pub fn smi_mgpu_ntt(m: *mut smi_mgpu, d_strip: *mut u32, d_out: *mut u32, log_n: u32, inverse: c_int, offset: u64) -> c_int;
    pub fn smi_mgpu_ntt_natural(m: *mut smi_mgpu, d_strip: *mut u32, d_out: *mut u32, log_n: u32, inverse: c_int, offset: u64) -> c_int;
    pub fn smi_mgpu_ntt_first_digit(log_n: u32, log_r0: *mut u32) -> c_int;
    pub fn smi_mgpu_stark_prove(m: *mut smi_mgpu, cfg: *const smi_stark_cfg, d_trace_cols: *const u32, column_roots: *mut u8, proof: *mut *mut u8, proof_len: *mut usize, top_indices: *mut u64) -> c_int;
}
// END GENERATED

// ------------------------------------------------------------------------------------------------
// Safe layer.  One context per thread (the C context is single-owner: `!Sync`, src: SURVEY 8b
// "Threading"); (998244353, 3) is the reference field (src/ff.rs:191-197, 215-223).

pub const P_REF: u64 = 998_244_353;
pub const G_REF: u64 = 3;

/// Owning handle of an `smi_ctx` (`smi_ctx_destroy` on drop).  Not `Send`/`Sync`: raw pointer inside.
pub struct Context {
    raw: *mut smi_ctx,
}

impl Context {
    /// `smi_ctx_create(p, g, device)`; panics with the library's message when there is no GPU or the
    /// modulus is unsupported -- there is no CPU fallback behind this boundary.
    pub fn new(p: u64, g: u64, device: i32) -> Context {
        let mut raw: *mut smi_ctx = std::ptr::null_mut();
        check(unsafe { smi_ctx_create(p, g, device as c_int, &mut raw) });
        Context { raw }
    }
    pub fn reference_field() -> Context {
        Context::new(P_REF, G_REF, 0)
    }
    pub fn as_ptr(&self) -> *mut smi_ctx {
        self.raw
    }
    /// status -> panic with the reference's text, plus `smi_last_error` for the codes that carry detail
    pub fn check(&self, status: c_int) {
        if status == 0 {
            return;
        }
        let msg = status_text(status);
        if status <= SMI_ERR_BAD_ARG {
            let detail = unsafe { CStr::from_ptr(smi_last_error(self.raw)) }.to_string_lossy().into_owned();
            if !detail.is_empty() {
                panic!("{}: {}", msg, detail);
            }
        }
        panic!("{}", msg);
    }
}

impl Drop for Context {
    fn drop(&mut self) {
        unsafe { smi_ctx_destroy(self.raw) }
    }
}

thread_local! {
    static CTX: Context = Context::reference_field();
}

/// Runs `f` with this thread's context for the reference field.
pub fn with_ctx<R>(f: impl FnOnce(&Context) -> R) -> R {
    CTX.with(|c| f(c))
}

pub fn status_text(status: c_int) -> String {
    unsafe { CStr::from_ptr(smi_status_string(status)) }.to_string_lossy().into_owned()
}

/// A non-zero status becomes the reference's own panic: `smi_status_string` returns the identical message
/// ("no inverse", "Number of leaves must be power of 2", ...).
pub fn check(status: c_int) {
    if status != 0 {
        panic!("{}", status_text(status));
    }
}

fn log2_exact(n: usize) -> u32 {
    assert!(n.is_power_of_two(), "n must be a power of two");
    n.trailing_zeros()
}

/// `Some(offset)` when `domain` is `offset * omega^k` for the primitive `domain.len()`-th root the reference's
/// `prim_nth_root` returns -- the domains the transforms serve; `None` means "take `interpolate_points` /
/// `eval_points`".
pub fn geometric_offset(ctx: &Context, domain: &[u64]) -> Option<u64> {
    let mut offset = 0u64;
    match unsafe { smi_domain_is_geometric(ctx.raw, domain.as_ptr(), domain.len(), &mut offset) } {
        0 => Some(offset),
        SMI_ERR_NOT_GEOMETRIC => None,
        st => {
            ctx.check(st);
            None
        }
    }
}

/// `Polynomial::interpolate_domain` on a geometric domain: coefficients (ascending) of the polynomial through
/// `(offset * omega^k, values[k])`.  The caller keeps the reference's two asserts and its H8 shape rule
/// (all-zero values of length > 1 give an empty coefficient vector).
pub fn interpolate_domain(ctx: &Context, values: &[u64], offset: u64) -> Vec<u64> {
    let mut coeffs = vec![0u64; values.len()];
    ctx.check(unsafe { smi_intt(ctx.raw, values.as_ptr(), coeffs.as_mut_ptr(), log2_exact(values.len()), offset) });
    coeffs
}

/// `Polynomial::eval_domain` on `offset * <omega_N>`, `N = 2^log_n >= coeffs.len()`, in domain order.
pub fn eval_domain(ctx: &Context, coeffs: &[u64], log_n: u32, offset: u64) -> Vec<u64> {
    let mut evals = vec![0u64; 1usize << log_n];
    ctx.check(unsafe { smi_coset_ntt(ctx.raw, coeffs.as_ptr(), coeffs.len(), evals.as_mut_ptr(), log_n, offset) });
    evals
}

/// `Polynomial::scale`: coefficient i times factor^i.
pub fn scale(ctx: &Context, coeffs: &[u64], factor: u64) -> Vec<u64> {
    let mut out = vec![0u64; coeffs.len()];
    ctx.check(unsafe { smi_poly_scale(ctx.raw, coeffs.as_ptr(), coeffs.len(), factor, out.as_mut_ptr()) });
    out
}

/// `Polynomial::mul` (empty for a zero operand, as the reference returns).
pub fn mul(ctx: &Context, a: &[u64], b: &[u64]) -> Vec<u64> {
    let mut out = vec![0u64; (a.len() + b.len()).max(1)];
    let mut n_out = 0usize;
    ctx.check(unsafe { smi_poly_mul(ctx.raw, a.as_ptr(), a.len(), b.as_ptr(), b.len(), out.as_mut_ptr(), &mut n_out) });
    out.truncate(n_out);
    out
}

/// `Polynomial::div` -> (quotient, remainder); a zero divisor panics "No division by zero".
pub fn div(ctx: &Context, a: &[u64], b: &[u64]) -> (Vec<u64>, Vec<u64>) {
    let mut q = vec![0u64; a.len().max(1)];
    let mut r = vec![0u64; a.len().max(b.len()).max(1)];
    let (mut nq, mut nr) = (0usize, 0usize);
    ctx.check(unsafe {
        smi_poly_div(ctx.raw, a.as_ptr(), a.len(), b.as_ptr(), b.len(), q.as_mut_ptr(), &mut nq, r.as_mut_ptr(), &mut nr)
    });
    q.truncate(nq);
    r.truncate(nr);
    (q, r)
}

/// `Polynomial::zerofier` on any points (duplicates and 0 allowed): the n + 1 coefficients of prod (x - d), monic.
/// An empty domain panics as the reference does when it indexes `domain[0]`.
pub fn zerofier(ctx: &Context, domain: &[u64]) -> Vec<u64> {
    let mut out = vec![0u64; domain.len() + 1];
    ctx.check(unsafe { smi_poly_zerofier(ctx.raw, domain.as_ptr(), domain.len(), out.as_mut_ptr()) });
    out
}

/// `Polynomial::eval_domain` on any point list: `f(points[k])` in order (`coeffs` may be longer than `points`).
pub fn eval_points(ctx: &Context, coeffs: &[u64], points: &[u64]) -> Vec<u64> {
    let mut out = vec![0u64; points.len()];
    ctx.check(unsafe { smi_poly_eval_points(ctx.raw, coeffs.as_ptr(), coeffs.len(), points.as_ptr(), points.len(), out.as_mut_ptr()) });
    out
}

/// `Polynomial::interpolate_domain` on any domain of distinct points: `domain.len()` coefficients (trailing zeros
/// included).  A repeated point panics "no inverse" like the reference's `field.inv`; the caller keeps the
/// reference's two asserts and its H8 shape rule, as for `interpolate_domain`.
pub fn interpolate_points(ctx: &Context, domain: &[u64], values: &[u64]) -> Vec<u64> {
    assert!(domain.len() == values.len(), "assertion failed: domain.len() == values.len()");
    let mut out = vec![0u64; domain.len()];
    ctx.check(unsafe { smi_poly_interpolate_points(ctx.raw, domain.as_ptr(), values.as_ptr(), domain.len(), out.as_mut_ptr()) });
    out
}

/// `codeword.iter().map(|e| Hash::from_field_elements(&[e.value]))` in one call (src/fri.rs:118-121).
pub fn hash_leaves(ctx: &Context, elems: &[u64]) -> Vec<[u8; 32]> {
    let mut out = vec![[0u8; 32]; elems.len()];
    ctx.check(unsafe { smi_hash_leaves(ctx.raw, elems.as_ptr(), elems.len(), out.as_mut_ptr() as *mut u8) });
    out
}

/// `Hash::combine` over adjacent pairs: out[i] = combine(digests[2i], digests[2i+1]).
pub fn combine_pairs(ctx: &Context, digests: &[[u8; 32]]) -> Vec<[u8; 32]> {
    let n_pairs = digests.len() / 2;
    let mut out = vec![[0u8; 32]; n_pairs];
    ctx.check(unsafe { smi_hash_combine_pairs(ctx.raw, digests.as_ptr() as *const u8, n_pairs, out.as_mut_ptr() as *mut u8) });
    out
}

/// `Hash::from_bytes` of one message.
pub fn hash_bytes(ctx: &Context, msg: &[u8]) -> [u8; 32] {
    let mut out = [0u8; 32];
    ctx.check(unsafe { smi_hash_bytes(ctx.raw, msg.as_ptr(), msg.len(), out.as_mut_ptr()) });
    out
}

/// `MerkleTree` with all levels resident on the device; `open` is a gather, nothing is rebuilt.
pub struct MerkleTree<'c> {
    ctx: &'c Context,
    raw: *mut smi_tree,
}

impl<'c> MerkleTree<'c> {
    /// `MerkleTree::new(&leaves)`: panics "Cannot create tree from empty leaves" / "Number of leaves must be power of 2".
    pub fn new(ctx: &'c Context, leaves: &[[u8; 32]]) -> MerkleTree<'c> {
        let mut raw: *mut smi_tree = std::ptr::null_mut();
        ctx.check(unsafe { smi_merkle_new(ctx.raw, leaves.as_ptr() as *const u8, leaves.len(), &mut raw) });
        MerkleTree { ctx, raw }
    }
    /// the same tree from the codeword itself (leaf hashing fused with the bottom levels)
    pub fn from_codeword(ctx: &'c Context, codeword: &[u64]) -> MerkleTree<'c> {
        let mut raw: *mut smi_tree = std::ptr::null_mut();
        ctx.check(unsafe { smi_merkle_from_codeword(ctx.raw, codeword.as_ptr(), codeword.len(), &mut raw) });
        MerkleTree { ctx, raw }
    }
    pub fn get_root(&self) -> [u8; 32] {
        let mut root = [0u8; 32];
        self.ctx.check(unsafe { smi_merkle_root(self.ctx.raw, self.raw, root.as_mut_ptr()) });
        root
    }
    /// `open(index)`: the sibling at each level, bottom up; panics "Index out of bounds".
    pub fn open(&self, index: usize) -> Vec<[u8; 32]> {
        let n = unsafe { smi_merkle_num_leaves(self.raw) };
        let mut path = vec![[0u8; 32]; (usize::BITS - n.leading_zeros()) as usize];
        let mut depth = 0usize;
        self.ctx.check(unsafe { smi_merkle_open(self.ctx.raw, self.raw, index, path.as_mut_ptr() as *mut u8, &mut depth) });
        path.truncate(depth);
        path
    }
    /// `nodes[level]` of the reference's struct, on demand
    pub fn level(&self, level: u32) -> Vec<[u8; 32]> {
        let n = unsafe { smi_merkle_num_leaves(self.raw) } >> level;
        let mut out = vec![[0u8; 32]; n.max(1)];
        let mut n_out = 0usize;
        self.ctx.check(unsafe { smi_merkle_level(self.ctx.raw, self.raw, level, out.as_mut_ptr() as *mut u8, &mut n_out) });
        out.truncate(n_out);
        out
    }
    /// `MerkleTree::commit(&leaves)` without keeping the tree
    pub fn commit(ctx: &Context, leaves: &[[u8; 32]]) -> [u8; 32] {
        let mut root = [0u8; 32];
        ctx.check(unsafe { smi_merkle_commit(ctx.raw, leaves.as_ptr() as *const u8, leaves.len(), root.as_mut_ptr()) });
        root
    }
}

impl Drop for MerkleTree<'_> {
    fn drop(&mut self) {
        unsafe { smi_merkle_free(self.raw) }
    }
}

/// `Fri::new` checks (src/fri.rs:37-45) + the struct the entry points take.
pub fn fri_cfg(ctx: &Context, omega: u64, offset: u64, domain_length: u64, expansion_factor: u64, num_colinearity_tests: u64) -> smi_fri_cfg {
    let cfg = smi_fri_cfg { omega, offset, domain_length, expansion_factor, num_colinearity_tests };
    ctx.check(unsafe { smi_fri_check(ctx.raw, &cfg) });
    cfg
}

/// `Fri::fold_codeword(codeword, alpha, offset, omega)`; alpha is passed unreduced, as `FiatShamir::challenge` makes it.
pub fn fold_codeword(ctx: &Context, codeword: &[u64], alpha: u64, offset: u64, omega: u64) -> Vec<u64> {
    let mut out = vec![0u64; codeword.len() / 2];
    ctx.check(unsafe { smi_fri_fold(ctx.raw, codeword.as_ptr(), codeword.len(), alpha, offset, omega, out.as_mut_ptr()) });
    out
}

/// `Fri::prove` with a fresh `FiatShamir` and `ProofStream`: (`ProofStream::serialize()` bytes, top-level indices).
/// The caller deserializes, pushes the objects and absorbs the roots to leave its own objects as the reference does.
pub fn fri_prove(ctx: &Context, cfg: &smi_fri_cfg, codeword: &[u64]) -> (Vec<u8>, Vec<usize>) {
    let mut proof: *mut u8 = std::ptr::null_mut();
    let mut len = 0usize;
    let mut top = vec![0u64; (cfg.num_colinearity_tests as usize).max(1)];
    ctx.check(unsafe { smi_fri_prove(ctx.raw, cfg, codeword.as_ptr(), codeword.len(), &mut proof, &mut len, top.as_mut_ptr()) });
    let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
    unsafe { smi_free(proof as *mut c_void) };
    top.truncate(cfg.num_colinearity_tests as usize);
    (bytes, top.into_iter().map(|v| v as usize).collect())
}

/// `Fri::verify` of a serialized stream against a fresh transcript: (verdict, the (index, value) pairs the
/// reference pushes to `polynomial_values`).  `Err(())` = the last layer's domain is not a coset of roots of
/// unity (SMI_ERR_NOT_GEOMETRIC): run the CPU body instead.  A reference panic panics here with the same text.
pub fn fri_verify(ctx: &Context, cfg: &smi_fri_cfg, proof: &[u8]) -> Result<(bool, Vec<(usize, u64)>), ()> {
    let t = cfg.num_colinearity_tests as usize;
    let (mut idx, mut val) = (vec![0u64; 2 * t + 2], vec![0u64; 2 * t + 2]);
    let (mut accept, mut n) = (0 as c_int, 0usize);
    let st = unsafe { smi_fri_verify(ctx.raw, cfg, proof.as_ptr(), proof.len(), &mut accept, idx.as_mut_ptr(), val.as_mut_ptr(), &mut n) };
    if st == SMI_ERR_NOT_GEOMETRIC {
        return Err(());
    }
    ctx.check(st);
    Ok((accept != 0, (0..n).map(|i| (idx[i] as usize, val[i])).collect()))
}

/// The roots at the head of `objs` (serialized MerkleRoot objects, at most the cfg's round count) appended to the
/// caller's transcript: what `fiat_shamir.absorb(&root.0)` leaves behind in `Fri::commit` / `Fri::verify`
/// (src/fri.rs:131, :328), in both cases for every root it got to.
fn absorb_roots(cfg: &smi_fri_cfg, objs: &[u8], transcript: &mut Vec<u8>) {
    let mut rounds = 0u64;
    check(unsafe { smi_fri_num_rounds(cfg, &mut rounds) });
    for k in 0..rounds as usize {
        let at = 33 * k;
        if objs.len() < at + 33 || objs[at] != 0 {
            break;
        }
        transcript.extend_from_slice(&objs[at + 1..at + 33]);
    }
}

/// `Fri::commit(codeword, proof_stream, fiat_shamir)` (src/fri.rs:105-156) continuing the caller's objects:
/// `transcript` is `fiat_shamir.transcript`, `stream` the caller's `ProofStream::serialize()` bytes so far.  Appends
/// the roots and the last codeword to `stream`, absorbs the roots into `transcript`, and returns (roots, the R-1
/// unreduced challenges, the last codeword).
pub fn fri_commit_with(ctx: &Context, cfg: &smi_fri_cfg, codeword: &[u64], transcript: &mut Vec<u8>, stream: &mut Vec<u8>)
                       -> (Vec<[u8; 32]>, Vec<u64>, Vec<u64>) {
    let mut rounds = 0u64;
    check(unsafe { smi_fri_num_rounds(cfg, &mut rounds) });
    let r = (rounds as usize).max(1);
    let (mut roots, mut alphas, mut last) = (vec![0u8; 32 * r], vec![0u64; r], vec![0u64; codeword.len()]);
    let mut last_len = 0usize;
    ctx.check(unsafe {
        smi_fri_commit_fs(ctx.raw, cfg, transcript.as_ptr(), transcript.len(), codeword.as_ptr(), codeword.len(), roots.as_mut_ptr(),
                          alphas.as_mut_ptr(), last.as_mut_ptr(), &mut last_len, std::ptr::null_mut())
    });
    let roots: Vec<[u8; 32]> = (0..rounds as usize).map(|k| roots[32 * k..32 * k + 32].try_into().unwrap()).collect();
    last.truncate(last_len);
    for root in &roots {                                                    // src/fri.rs:129-131, src/stream.rs:39-42
        stream.push(0);
        stream.extend_from_slice(root);
        transcript.extend_from_slice(root);
    }
    stream.push(2);                                                         // src/fri.rs:151, src/stream.rs:48-53
    stream.extend_from_slice(&(last.len() as u64).to_le_bytes());
    for v in &last {
        stream.extend_from_slice(&v.to_le_bytes());
    }
    alphas.truncate((rounds as usize).saturating_sub(1));
    (roots, alphas, last)
}

/// `Fri::prove(codeword, fiat_shamir, proof_stream)` (src/fri.rs:250-311) continuing the caller's objects: `transcript`
/// and `stream` as in `fri_commit_with`.  Appends the objects Fri::prove pushes to `stream`, absorbs the roots into
/// `transcript` and returns the top-level indices.
pub fn fri_prove_with(ctx: &Context, cfg: &smi_fri_cfg, codeword: &[u64], transcript: &mut Vec<u8>, stream: &mut Vec<u8>) -> Vec<usize> {
    let mut proof: *mut u8 = std::ptr::null_mut();
    let mut len = 0usize;
    let mut top = vec![0u64; (cfg.num_colinearity_tests as usize).max(1)];
    ctx.check(unsafe {
        smi_fri_prove_fs(ctx.raw, cfg, transcript.as_ptr(), transcript.len(), codeword.as_ptr(), codeword.len(), &mut proof, &mut len,
                         top.as_mut_ptr())
    });
    let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
    unsafe { smi_free(proof as *mut c_void) };
    absorb_roots(cfg, &bytes, transcript);
    stream.extend_from_slice(&bytes);
    top.truncate(cfg.num_colinearity_tests as usize);
    top.into_iter().map(|v| v as usize).collect()
}

/// `Fri::verify(proof_stream, fiat_shamir, polynomial_values)` (src/fri.rs:313-504) continuing the caller's objects:
/// `transcript` is `fiat_shamir.transcript`, `stream` the serialized objects still to be popped.  Absorbs the roots it
/// pops into `transcript` and returns (verdict, the (index, value) pairs, the bytes of the objects it popped -- on
/// acceptance; the caller goes on from there).  `Err(())` as in `fri_verify`.
pub fn fri_verify_with(ctx: &Context, cfg: &smi_fri_cfg, transcript: &mut Vec<u8>, stream: &[u8])
                       -> Result<(bool, Vec<(usize, u64)>, usize), ()> {
    let t = cfg.num_colinearity_tests as usize;
    let (mut idx, mut val) = (vec![0u64; 2 * t + 2], vec![0u64; 2 * t + 2]);
    let (mut accept, mut n, mut consumed) = (0 as c_int, 0usize, 0usize);
    let st = unsafe {
        smi_fri_verify_fs(ctx.raw, cfg, transcript.as_ptr(), transcript.len(), stream.as_ptr(), stream.len(), &mut accept, idx.as_mut_ptr(),
                          val.as_mut_ptr(), &mut n, &mut consumed)
    };
    if st == SMI_ERR_NOT_GEOMETRIC {
        return Err(());
    }
    ctx.check(st);
    absorb_roots(cfg, stream, transcript);
    Ok((accept != 0, (0..n).map(|i| (idx[i] as usize, val[i])).collect(), consumed))
}

/// `Trace::to_field_elements` for all columns at once: row-major i128 rows (`Vec<Vec<i128>>` flattened) to
/// column-major u64 residues.
pub fn trace_pack(ctx: &Context, rows: &[i128], n_rows: usize, n_cols: usize) -> Vec<u64> {
    assert!(rows.len() == n_rows * n_cols);
    let mut cols = vec![0u64; n_rows * n_cols];
    ctx.check(unsafe { smi_trace_pack(ctx.raw, rows.as_ptr() as *const c_void, n_rows, n_cols, cols.as_mut_ptr()) });
    cols
}

/// Low-degree extension of `n_cols` columns (column-major, 2^log_n rows each): interpolate on
/// `trace_offset * <omega_n>`, evaluate on `lde_offset * <omega_N>`, N = n << log_blowup.
pub fn lde(ctx: &Context, cols: &[u64], n_cols: u32, log_n: u32, log_blowup: u32, trace_offset: u64, lde_offset: u64) -> Vec<u64> {
    assert!(cols.len() == (n_cols as usize) << log_n);
    let mut out = vec![0u64; (n_cols as usize) << (log_n + log_blowup)];
    ctx.check(unsafe { smi_lde(ctx.raw, cols.as_ptr(), n_cols, log_n, log_blowup, trace_offset, lde_offset, out.as_mut_ptr()) });
    out
}

/// An AIR over `n_cols` trace columns (include/stark_mi.h, "AIR"): boundary points and transition constraints,
/// flattened to `smi_air` for the duration of a call.  The reference has no counterpart (its `Trace` has no
/// consumer); this is where a `Stark::prove` would call.
#[derive(Clone, Debug, Default)]
pub struct Air {
    pub n_cols: u32,
    constraint_first_term: Vec<u32>,
    term_coeff: Vec<u64>,
    term_first_factor: Vec<u32>,
    factor_var: Vec<u32>,
    factor_exp: Vec<u32>,
    boundary_col: Vec<u32>,
    boundary_row: Vec<u64>,
    boundary_value: Vec<u64>,
    periodic_log_period: Vec<u32>,
    periodic_value: Vec<u64>,
}

/// One factor of a monomial: column, row shift (0 = this row, 1 = next row), exponent.  `AirFactor::periodic` names a
/// periodic column in place of a trace column.
#[derive(Clone, Copy, Debug)]
pub struct AirFactor {
    pub col: u32,
    pub next: bool,
    pub exp: u32,
}

/// Set in `AirFactor::col` when the factor is a periodic column (the rest is the index `Air::periodic` returned).
pub const AIR_PERIODIC: u32 = 1 << 31;

impl AirFactor {
    /// Periodic column `j` (as returned by `Air::periodic`) at this row or the next.
    pub fn periodic(j: u32, next: bool, exp: u32) -> AirFactor {
        AirFactor { col: AIR_PERIODIC | j, next, exp }
    }
}

impl Air {
    pub fn new(n_cols: u32) -> Air {
        Air { n_cols, constraint_first_term: vec![0], term_first_factor: vec![0], ..Default::default() }
    }
    /// Column `col` holds `value` (canonical) in row `row`.
    pub fn boundary(&mut self, col: u32, row: u64, value: u64) -> &mut Air {
        self.boundary_col.push(col);
        self.boundary_row.push(row);
        self.boundary_value.push(value);
        self
    }
    /// A periodic column: row r holds `values[r mod values.len()]` (canonical; the length a power of two that divides
    /// the trace length).  Part of the statement: not committed, not in the proof.  Returns its index for
    /// `AirFactor::periodic`.
    pub fn periodic(&mut self, values: &[u64]) -> u32 {
        assert!(values.len().is_power_of_two(), "the period must be a power of two");
        self.periodic_log_period.push(values.len().trailing_zeros());
        self.periodic_value.extend_from_slice(values);
        (self.periodic_log_period.len() - 1) as u32
    }
    /// One transition constraint: a sum of `(coefficient, factors)` terms that vanishes on every pair of consecutive rows.
    pub fn transition(&mut self, terms: &[(u64, Vec<AirFactor>)]) -> &mut Air {
        for (coeff, factors) in terms {
            self.term_coeff.push(*coeff);
            for f in factors {
                // a periodic factor keeps its tag until with_raw, where the number of periodic columns is final
                self.factor_var.push(if f.col & AIR_PERIODIC != 0 { f.col | if f.next { AIR_PERIODIC >> 1 } else { 0 } }
                                     else { f.col + if f.next { self.n_cols } else { 0 } });
                self.factor_exp.push(f.exp);
            }
            self.term_first_factor.push(self.factor_var.len() as u32);
        }
        self.constraint_first_term.push(self.term_coeff.len() as u32);
        self
    }
    fn with_raw<R>(&self, f: impl FnOnce(*const c_void) -> R) -> R {
        // var = 2W + j (this row) or 2W + Q + j (next row) for periodic column j
        let q = self.periodic_log_period.len() as u32;
        let factor_var: Vec<u32> = self.factor_var.iter().map(|&v| {
            if v & AIR_PERIODIC == 0 { v }
            else { 2 * self.n_cols + (v & !(AIR_PERIODIC | AIR_PERIODIC >> 1)) + if v & (AIR_PERIODIC >> 1) != 0 { q } else { 0 } }
        }).collect();
        let raw = smi_air {
            n_constraints: (self.constraint_first_term.len() - 1) as u32,
            n_terms: self.term_coeff.len() as u32,
            n_factors: self.factor_var.len() as u32,
            n_boundary: self.boundary_col.len() as u32,
            constraint_first_term: self.constraint_first_term.as_ptr(),
            term_coeff: self.term_coeff.as_ptr(),
            term_first_factor: self.term_first_factor.as_ptr(),
            factor_var: factor_var.as_ptr(),
            factor_exp: self.factor_exp.as_ptr(),
            boundary_col: self.boundary_col.as_ptr(),
            boundary_row: self.boundary_row.as_ptr(),
            boundary_value: self.boundary_value.as_ptr(),
            n_periodic: q,
            window: 0,   // two rows; a wider window is built on the raw struct ("AIR: transition windows")
            periodic_log_period: self.periodic_log_period.as_ptr(),
            periodic_value: self.periodic_value.as_ptr(),
        };
        f(&raw as *const smi_air as *const c_void)
    }
    /// `smi_air_plan` (host only): `(degree, FRI expansion factor)`; panics naming the limit that was broken.
    pub fn plan(&self, p: u64, cfg: &smi_stark_cfg) -> (u32, u64) {
        let (mut d, mut e) = (0u32, 0u64);
        let st = self.with_raw(|a| unsafe { smi_air_plan(p, cfg, a, &mut d, &mut e) });
        if st != 0 {
            let why = unsafe { CStr::from_ptr(smi_air_last_error()) }.to_string_lossy().into_owned();
            panic!("{}: {}", status_text(st), why);
        }
        (d, e)
    }
    /// `smi_dev_air_check`: `None` when the device trace satisfies the AIR, else `(constraint, row)` of the first
    /// violation (boundary points first; a transition constraint k is reported as `n_boundary + k`).
    pub fn check_trace(&self, ctx: &Context, log_n: u32, d_trace_cols: *const u32) -> Option<(u32, u64)> {
        let (mut ok, mut con, mut row) = (0 as c_int, 0u32, 0u64);
        ctx.check(self.with_raw(|a| unsafe { smi_dev_air_check(ctx.raw, a, self.n_cols, log_n, d_trace_cols, &mut ok, &mut con, &mut row) }));
        if ok != 0 { None } else { Some((con, row)) }
    }
    /// `smi_dev_air_compose`: the composition codeword of the extended device columns under `n_cols + K` device weights.
    pub fn compose(&self, ctx: &Context, cfg: &smi_stark_cfg, d_lde: *const u32, stride: usize, d_weights: *const u64, d_out: *mut u32) {
        ctx.check(self.with_raw(|a| unsafe { smi_dev_air_compose(ctx.raw, cfg, a, d_lde, stride, d_weights, d_out) }));
    }
    /// `smi_dev_air_prove` -> (column roots, proof bytes).  `check_trace` (the default a caller should pass: true)
    /// runs `smi_dev_air_check` first and panics naming the first violated constraint and row.
    pub fn prove(&self, ctx: &Context, cfg: &smi_stark_cfg, d_trace_cols: *const u32, check_trace: bool) -> (Vec<[u8; 32]>, Vec<u8>) {
        if check_trace {
            if let Some((con, row)) = self.check_trace(ctx, cfg.log_n, d_trace_cols) {
                let why = unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned();
                panic!("the trace violates constraint {} at row {}: {}", con, row, why);
            }
        }
        let mut roots = vec![[0u8; 32]; cfg.n_cols as usize];
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        ctx.check(self.with_raw(|a| unsafe {
            smi_dev_air_prove(ctx.raw, cfg, a, d_trace_cols, roots.as_mut_ptr() as *mut u8, &mut proof, &mut len, std::ptr::null_mut(), std::ptr::null_mut())
        }));
        let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { smi_free(proof as *mut c_void) };
        (roots, bytes)
    }
    /// `smi_air_verify` -> `Ok(())` or the reason the proof is rejected.
    pub fn verify(&self, ctx: &Context, cfg: &smi_stark_cfg, column_roots: &[[u8; 32]], proof: &[u8]) -> Result<(), String> {
        let mut accept = 0 as c_int;
        ctx.check(self.with_raw(|a| unsafe {
            smi_air_verify(ctx.raw, cfg, a, column_roots.as_ptr() as *const u8, proof.as_ptr(), proof.len(), &mut accept)
        }));
        if accept != 0 {
            Ok(())
        } else {
            Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned())
        }
    }
    /// `smi_dev_air_prove_rows` -> (root of the one tree over the rows, proof bytes): the same statement with every
    /// queried position opened once.  `check_trace` as in `prove`.
    pub fn prove_rows(&self, ctx: &Context, cfg: &smi_stark_cfg, d_trace_cols: *const u32, check_trace: bool) -> ([u8; 32], Vec<u8>) {
        if check_trace {
            if let Some((con, row)) = self.check_trace(ctx, cfg.log_n, d_trace_cols) {
                let why = unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned();
                panic!("the trace violates constraint {} at row {}: {}", con, row, why);
            }
        }
        let mut root = [0u8; 32];
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        ctx.check(self.with_raw(|a| unsafe {
            smi_dev_air_prove_rows(ctx.raw, cfg, a, d_trace_cols, root.as_mut_ptr(), &mut proof, &mut len, std::ptr::null_mut(), std::ptr::null_mut())
        }));
        let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { smi_free(proof as *mut c_void) };
        (root, bytes)
    }
    /// `smi_air_verify_rows` -> `Ok(())` or the reason the proof is rejected.
    pub fn verify_rows(&self, ctx: &Context, cfg: &smi_stark_cfg, row_root: &[u8; 32], proof: &[u8]) -> Result<(), String> {
        let mut accept = 0 as c_int;
        ctx.check(self.with_raw(|a| unsafe {
            smi_air_verify_rows(ctx.raw, cfg, a, row_root.as_ptr(), proof.as_ptr(), proof.len(), &mut accept)
        }));
        if accept != 0 {
            Ok(())
        } else {
            Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned())
        }
    }
    /// `smi_dev_air_prove_ext` -> (root of the one tree over the rows, proof bytes): the row-committed proof with the
    /// composition weights and FRI's challenges drawn from the quartic extension.  `check_trace` as in `prove`.
    pub fn prove_ext(&self, ctx: &Context, cfg: &smi_stark_cfg, d_trace_cols: *const u32, check_trace: bool) -> ([u8; 32], Vec<u8>) {
        if check_trace {
            if let Some((con, row)) = self.check_trace(ctx, cfg.log_n, d_trace_cols) {
                let why = unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned();
                panic!("the trace violates constraint {} at row {}: {}", con, row, why);
            }
        }
        let mut root = [0u8; 32];
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        ctx.check(self.with_raw(|a| unsafe {
            smi_dev_air_prove_ext(ctx.raw, cfg, a, d_trace_cols, root.as_mut_ptr(), &mut proof, &mut len, std::ptr::null_mut(), std::ptr::null_mut())
        }));
        let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { smi_free(proof as *mut c_void) };
        (root, bytes)
    }
    /// `smi_air_verify_ext` -> `Ok(())` or the reason the proof is rejected.
    pub fn verify_ext(&self, ctx: &Context, cfg: &smi_stark_cfg, row_root: &[u8; 32], proof: &[u8]) -> Result<(), String> {
        let mut accept = 0 as c_int;
        ctx.check(self.with_raw(|a| unsafe {
            smi_air_verify_ext(ctx.raw, cfg, a, row_root.as_ptr(), proof.as_ptr(), proof.len(), &mut accept)
        }));
        if accept != 0 {
            Ok(())
        } else {
            Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned())
        }
    }
    /// `smi_dev_air_prove_ext_pow` -> (root of the one tree over the rows, proof bytes): `prove_ext` with `grind_bits`
    /// proof-of-work bits ground before the query indices are drawn (17 bytes more).  `check_trace` as in `prove`.
    pub fn prove_ext_pow(&self, ctx: &Context, cfg: &smi_stark_cfg, d_trace_cols: *const u32, check_trace: bool, grind_bits: u32) -> ([u8; 32], Vec<u8>) {
        if check_trace {
            if let Some((con, row)) = self.check_trace(ctx, cfg.log_n, d_trace_cols) {
                let why = unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned();
                panic!("the trace violates constraint {} at row {}: {}", con, row, why);
            }
        }
        let mut root = [0u8; 32];
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        ctx.check(self.with_raw(|a| unsafe {
            smi_dev_air_prove_ext_pow(ctx.raw, cfg, a, d_trace_cols, root.as_mut_ptr(), &mut proof, &mut len, std::ptr::null_mut(), std::ptr::null_mut(), grind_bits)
        }));
        let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { smi_free(proof as *mut c_void) };
        (root, bytes)
    }
    /// `smi_air_verify_ext_pow` -> `Ok(())` or the reason the proof is rejected; `grind_bits` is the least difficulty
    /// demanded (a proof ground at more bits is accepted).
    pub fn verify_ext_pow(&self, ctx: &Context, cfg: &smi_stark_cfg, row_root: &[u8; 32], proof: &[u8], grind_bits: u32) -> Result<(), String> {
        let mut accept = 0 as c_int;
        ctx.check(self.with_raw(|a| unsafe {
            smi_air_verify_ext_pow(ctx.raw, cfg, a, row_root.as_ptr(), proof.as_ptr(), proof.len(), &mut accept, grind_bits)
        }));
        if accept != 0 {
            Ok(())
        } else {
            Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned())
        }
    }
    /// `smi_air_plan_perm` (host only): `(max(degree, 2), FRI expansion factor)` of this AIR with the permutation `perm`.
    pub fn plan_perm(&self, p: u64, cfg: &smi_stark_cfg, perm: &Permutation) -> (u32, u64) {
        let (mut d, mut e) = (0u32, 0u64);
        let st = self.with_raw(|a| perm.with_raw(|pm| unsafe { smi_air_plan_perm(p, cfg, a, pm, &mut d, &mut e) }));
        if st != SMI_OK {
            panic!("{}: {}", status_text(st), unsafe { CStr::from_ptr(smi_air_last_error()) }.to_string_lossy());
        }
        (d, e)
    }
    /// `smi_dev_air_prove_perm` -> (root_1 then root_2, proof bytes, closes): the AIR proof with the permutation argument
    /// `perm` over a committed extension column.  A trace whose product does not close is proved all the same (`closes`
    /// is false and the verifier rejects); a zero denominator panics with "no inverse" and the row.
    pub fn prove_perm(&self, ctx: &Context, cfg: &smi_stark_cfg, perm: &Permutation, d_trace_cols: *const u32, grind_bits: u32) -> ([u8; 64], Vec<u8>, bool) {
        let mut roots = [0u8; 64];
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        let mut closes = 0 as c_int;
        ctx.check(self.with_raw(|a| perm.with_raw(|pm| unsafe {
            smi_dev_air_prove_perm(ctx.raw, cfg, a, pm, d_trace_cols, roots.as_mut_ptr(), &mut proof, &mut len, std::ptr::null_mut(), std::ptr::null_mut(), grind_bits, &mut closes)
        })));
        let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { smi_free(proof as *mut c_void) };
        (roots, bytes, closes != 0)
    }
    /// `smi_air_verify_perm` -> `Ok(())` or the reason the proof is rejected.
    pub fn verify_perm(&self, ctx: &Context, cfg: &smi_stark_cfg, perm: &Permutation, roots: &[u8; 64], proof: &[u8], grind_bits: u32) -> Result<(), String> {
        let mut accept = 0 as c_int;
        ctx.check(self.with_raw(|a| perm.with_raw(|pm| unsafe {
            smi_air_verify_perm(ctx.raw, cfg, a, pm, roots.as_ptr(), proof.as_ptr(), proof.len(), &mut accept, grind_bits)
        })));
        if accept != 0 {
            Ok(())
        } else {
            Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned())
        }
    }
    /// `smi_air_plan_lookup` (host only): `(max(degree, 3), FRI expansion factor)` of this AIR with the lookup `lookup`.
    pub fn plan_lookup(&self, p: u64, cfg: &smi_stark_cfg, lookup: &Lookup) -> (u32, u64) {
        let (mut d, mut e) = (0u32, 0u64);
        let st = self.with_raw(|a| lookup.with_raw(|lk| unsafe { smi_air_plan_lookup(p, cfg, a, lk, &mut d, &mut e) }));
        if st != SMI_OK {
            panic!("{}: {}", status_text(st), unsafe { CStr::from_ptr(smi_air_last_error()) }.to_string_lossy());
        }
        (d, e)
    }
    /// `smi_dev_air_prove_lookup` -> (root_1 then root_2, proof bytes, closes): the AIR proof with the lookup argument
    /// `lookup` over a committed extension column; the trace's multiplicity column is taken as filled
    /// (`Lookup::multiplicities`).  A trace whose sum does not close is proved all the same (`closes` is false and the
    /// verifier rejects); a zero denominator panics with "no inverse" and the row.
    pub fn prove_lookup(&self, ctx: &Context, cfg: &smi_stark_cfg, lookup: &Lookup, d_trace_cols: *const u32, grind_bits: u32) -> ([u8; 64], Vec<u8>, bool) {
        let mut roots = [0u8; 64];
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        let mut closes = 0 as c_int;
        ctx.check(self.with_raw(|a| lookup.with_raw(|lk| unsafe {
            smi_dev_air_prove_lookup(ctx.raw, cfg, a, lk, d_trace_cols, roots.as_mut_ptr(), &mut proof, &mut len, std::ptr::null_mut(), std::ptr::null_mut(), grind_bits, &mut closes)
        })));
        let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { smi_free(proof as *mut c_void) };
        (roots, bytes, closes != 0)
    }
    /// `smi_air_verify_lookup` -> `Ok(())` or the reason the proof is rejected.
    pub fn verify_lookup(&self, ctx: &Context, cfg: &smi_stark_cfg, lookup: &Lookup, roots: &[u8; 64], proof: &[u8], grind_bits: u32) -> Result<(), String> {
        let mut accept = 0 as c_int;
        ctx.check(self.with_raw(|a| lookup.with_raw(|lk| unsafe {
            smi_air_verify_lookup(ctx.raw, cfg, a, lk, roots.as_ptr(), proof.as_ptr(), proof.len(), &mut accept, grind_bits)
        })));
        if accept != 0 {
            Ok(())
        } else {
            Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned())
        }
    }
    /// `smi_dev_air_compose_lookup`: the composition under the first 4 (W + K) of the 4 (W + K + 2) device weights plus the
    /// two auxiliary quotients of the extended column `d_s_lde`, into four coordinate columns `out_stride` apart.
    pub fn compose_lookup(&self, ctx: &Context, cfg: &smi_stark_cfg, lookup: &Lookup, d_lde: *const u32, stride: usize, d_s_lde: *const u32, s_stride: usize,
                          challenges: &[u64; 8], d_weights: *const u64, d_out: *mut u32, out_stride: usize) {
        ctx.check(self.with_raw(|a| lookup.with_raw(|lk| unsafe {
            smi_dev_air_compose_lookup(ctx.raw, cfg, a, lk, d_lde, stride, d_s_lde, s_stride, challenges.as_ptr(), d_weights, d_out, out_stride)
        })));
    }
    /// `smi_air_plan_args` (host only): `(degree, FRI expansion factor)` of this AIR with the argument list `args`.
    pub fn plan_args(&self, p: u64, cfg: &smi_stark_cfg, args: &Arguments) -> (u32, u64) {
        let (mut d, mut e) = (0u32, 0u64);
        let st = self.with_raw(|a| args.with_raw(|al| unsafe { smi_air_plan_args(p, cfg, a, al, &mut d, &mut e) }));
        if st != SMI_OK {
            panic!("{}: {}", status_text(st), unsafe { CStr::from_ptr(smi_air_last_error()) }.to_string_lossy());
        }
        (d, e)
    }
    /// `smi_dev_air_prove_args` -> (root_1 then root_2, proof bytes, closes): one AIR proof with every argument of `args`
    /// over one second tree; bit a of `closes` is set iff argument a closes.  A column that does not close is proved all the
    /// same and the verifier rejects; a zero denominator panics with "no inverse", the argument and the row.
    pub fn prove_args(&self, ctx: &Context, cfg: &smi_stark_cfg, args: &Arguments, d_trace_cols: *const u32, grind_bits: u32) -> ([u8; 64], Vec<u8>, u32) {
        let mut roots = [0u8; 64];
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        let mut closes = 0u32;
        ctx.check(self.with_raw(|a| args.with_raw(|al| unsafe {
            smi_dev_air_prove_args(ctx.raw, cfg, a, al, d_trace_cols, roots.as_mut_ptr(), &mut proof, &mut len, std::ptr::null_mut(), std::ptr::null_mut(), grind_bits, &mut closes)
        })));
        let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { smi_free(proof as *mut c_void) };
        (roots, bytes, closes)
    }
    /// `smi_air_verify_args` -> `Ok(())` or the reason the proof is rejected.
    pub fn verify_args(&self, ctx: &Context, cfg: &smi_stark_cfg, args: &Arguments, roots: &[u8; 64], proof: &[u8], grind_bits: u32) -> Result<(), String> {
        let mut accept = 0 as c_int;
        ctx.check(self.with_raw(|a| args.with_raw(|al| unsafe {
            smi_air_verify_args(ctx.raw, cfg, a, al, roots.as_ptr(), proof.as_ptr(), proof.len(), &mut accept, grind_bits)
        })));
        if accept != 0 {
            Ok(())
        } else {
            Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned())
        }
    }
    /// `smi_dev_air_compose_args`: the composition under the first 4 (W + K) of the 4 (W + K + 2 A) device weights plus the
    /// 2 A auxiliary quotients of the 4 A extended coordinate columns `d_c_lde`, into four coordinate columns.
    pub fn compose_args(&self, ctx: &Context, cfg: &smi_stark_cfg, args: &Arguments, d_lde: *const u32, stride: usize, d_c_lde: *const u32, c_stride: usize,
                        challenges: &[u64; 8], d_weights: *const u64, d_out: *mut u32, out_stride: usize) {
        ctx.check(self.with_raw(|a| args.with_raw(|al| unsafe {
            smi_dev_air_compose_args(ctx.raw, cfg, a, al, d_lde, stride, d_c_lde, c_stride, challenges.as_ptr(), d_weights, d_out, out_stride)
        })));
    }
}

/// An argument list (include/stark_mi.h, "Argument list"): 1 ..= `SMI_ARGS_MAX` permutations and lookups, in any mix and
/// order, proved over one committed trace with one second tree.
pub struct Arguments {
    items: Vec<(u32, Vec<u32>, Vec<u32>, u32)>,   // kind, a_col, b_col, mult_col
}

impl Arguments {
    pub fn new() -> Arguments {
        Arguments { items: Vec::new() }
    }
    pub fn permutation(mut self, left: &[u32], right: &[u32]) -> Arguments {
        assert!(left.len() == right.len() && !left.is_empty() && left.len() <= SMI_PERM_MAX_WIDTH as usize, "1 ..= SMI_PERM_MAX_WIDTH columns a side");
        assert!(self.items.len() < SMI_ARGS_MAX as usize, "at most SMI_ARGS_MAX arguments");
        self.items.push((SMI_ARG_PERM, left.to_vec(), right.to_vec(), 0));
        self
    }
    pub fn lookup(mut self, lookup: &[u32], table: &[u32], mult_col: u32) -> Arguments {
        assert!(lookup.len() == table.len() && !lookup.is_empty() && lookup.len() <= SMI_LOOKUP_MAX_WIDTH as usize, "1 ..= SMI_LOOKUP_MAX_WIDTH columns a side");
        assert!(self.items.len() < SMI_ARGS_MAX as usize, "at most SMI_ARGS_MAX arguments");
        self.items.push((SMI_ARG_LOOKUP, lookup.to_vec(), table.to_vec(), mult_col));
        self
    }
    fn with_raw<R>(&self, f: impl FnOnce(*const c_void) -> R) -> R {
        let raw: Vec<smi_air_arg> = self.items.iter().map(|(kind, a, b, m)| smi_air_arg { kind: *kind, width: a.len() as u32, mult_col: *m, reserved0: 0, a_col: a.as_ptr(), b_col: b.as_ptr() }).collect();
        let list = smi_air_args { count: raw.len() as u32, reserved0: 0, arg: raw.as_ptr() };
        f(&list as *const smi_air_args as *const c_void)
    }
    /// `smi_dev_args_columns`: the A columns of the device trace under the 8 unreduced challenges into 4 A coordinate
    /// columns `c_stride` apart -> the mask of the arguments that close.  Panics with "no inverse" when a denominator is zero.
    pub fn columns(&self, ctx: &Context, d_trace_cols: *const u32, n_cols: u32, log_n: u32, challenges: &[u64; 8], d_c: *mut u32, c_stride: usize) -> u32 {
        let mut closes = 0u32;
        ctx.check(self.with_raw(|al| unsafe {
            smi_dev_args_columns(ctx.raw, al, d_trace_cols, n_cols, log_n, challenges.as_ptr(), d_c, c_stride, &mut closes)
        }));
        closes
    }
}

/// A member or selector of an argument with selectors and periodic members: a trace column or a periodic column of the AIR.
#[derive(Clone, Copy)]
pub enum Operand {
    Col(u32),
    Periodic(u32),
}

/// An argument list with selectors and periodic members (include/stark_mi.h, "Argument list with selectors and periodic
/// members"): `Arguments` whose tuple members may be periodic columns of the AIR and whose sides may each have a selector.
/// `n_cols` is the trace width the operands are numbered against.
pub struct SelectedArguments {
    n_cols: u32,
    items: Vec<(u32, Vec<u32>, Vec<u32>, u32, u32, u32)>,   // kind, a_var, b_var, mult_col, a_sel, b_sel
}

impl SelectedArguments {
    pub fn new(n_cols: u32) -> SelectedArguments {
        SelectedArguments { n_cols, items: Vec::new() }
    }
    fn var(&self, o: Operand) -> u32 {
        match o {
            Operand::Col(c) => c,
            Operand::Periodic(j) => 2 * self.n_cols + j,
        }
    }
    fn sel(&self, o: Option<Operand>) -> u32 {
        o.map_or(SMI_ARG_NO_SELECTOR, |x| self.var(x))
    }
    pub fn permutation(mut self, left: &[Operand], right: &[Operand], left_sel: Option<Operand>, right_sel: Option<Operand>) -> SelectedArguments {
        assert!(left.len() == right.len() && !left.is_empty() && left.len() <= SMI_PERM_MAX_WIDTH as usize, "1 ..= SMI_PERM_MAX_WIDTH members a side");
        assert!(self.items.len() < SMI_ARGS_MAX as usize, "at most SMI_ARGS_MAX arguments");
        let item = (SMI_ARG_PERM, left.iter().map(|o| self.var(*o)).collect(), right.iter().map(|o| self.var(*o)).collect(), 0, self.sel(left_sel), self.sel(right_sel));
        self.items.push(item);
        self
    }
    pub fn lookup(mut self, lookup: &[Operand], table: &[Operand], mult_col: u32, sel: Option<Operand>, table_sel: Option<Operand>) -> SelectedArguments {
        assert!(lookup.len() == table.len() && !lookup.is_empty() && lookup.len() <= SMI_LOOKUP_MAX_WIDTH as usize, "1 ..= SMI_LOOKUP_MAX_WIDTH members a side");
        assert!(self.items.len() < SMI_ARGS_MAX as usize, "at most SMI_ARGS_MAX arguments");
        let item = (SMI_ARG_LOOKUP, lookup.iter().map(|o| self.var(*o)).collect(), table.iter().map(|o| self.var(*o)).collect(), mult_col, self.sel(sel), self.sel(table_sel));
        self.items.push(item);
        self
    }
    /// A shared-table lookup (include/stark_mi.h, "Shared-table lookups"): 1 ..= `SMI_ARG_MAX_TUPLES` looked-up tuples of one
    /// width, each with its own optional selector, into one table with one multiplicity column and one running sum.  One
    /// tuple is `lookup`.
    pub fn shared_lookup(mut self, tuples: &[&[Operand]], sels: &[Option<Operand>], table: &[Operand], mult_col: u32, table_sel: Option<Operand>) -> SelectedArguments {
        assert!(!tuples.is_empty() && tuples.len() <= SMI_ARG_MAX_TUPLES as usize && sels.len() == tuples.len(), "1 ..= SMI_ARG_MAX_TUPLES tuples, one selector or None each");
        assert!(!table.is_empty() && table.len() <= SMI_LOOKUP_MAX_WIDTH as usize && tuples.iter().all(|t| t.len() == table.len()), "tuples of the table's width, 1 ..= SMI_LOOKUP_MAX_WIDTH");
        if tuples.len() == 1 {
            return self.lookup(tuples[0], table, mult_col, sels[0], table_sel);
        }
        assert!(self.items.len() < SMI_ARGS_MAX as usize, "at most SMI_ARGS_MAX arguments");
        // a_var: the J m operands, tuple-major, then the J selector entries; J - 1 in the second byte of kind
        let mut a: Vec<u32> = tuples.iter().flat_map(|t| t.iter().map(|o| self.var(*o))).collect();
        a.extend(sels.iter().map(|x| self.sel(*x)));
        let kind = SMI_ARG_LOOKUP | ((tuples.len() as u32 - 1) << SMI_ARG_TUPLES_SHIFT);
        let item = (kind, a, table.iter().map(|o| self.var(*o)).collect(), mult_col, SMI_ARG_NO_SELECTOR, self.sel(table_sel));
        self.items.push(item);
        self
    }
    fn with_raw<R>(&self, f: impl FnOnce(*const c_void) -> R) -> R {
        let raw: Vec<smi_air_xarg> = self.items.iter().map(|(kind, a, b, m, sa, sb)| smi_air_xarg { kind: *kind, width: b.len() as u32, mult_col: *m, reserved0: 0, a_var: a.as_ptr(), b_var: b.as_ptr(), a_sel: *sa, b_sel: *sb }).collect();
        let list = smi_air_xargs { count: raw.len() as u32, reserved0: 0, arg: raw.as_ptr() };
        f(&list as *const smi_air_xargs as *const c_void)
    }
    /// `smi_air_plan_xargs` (host only): `(degree, FRI expansion factor)` of `air` with this list.
    pub fn plan(&self, air: &Air, p: u64, cfg: &smi_stark_cfg) -> (u32, u64) {
        let (mut d, mut e) = (0u32, 0u64);
        let st = air.with_raw(|a| self.with_raw(|al| unsafe { smi_air_plan_xargs(p, cfg, a, al, &mut d, &mut e) }));
        if st != SMI_OK {
            panic!("{}: {}", status_text(st), unsafe { CStr::from_ptr(smi_air_last_error()) }.to_string_lossy());
        }
        (d, e)
    }
    /// `smi_dev_xargs_multiplicities`: the multiplicities of lookup argument `a` over the selected rows into `d_mult`.
    pub fn multiplicities(&self, ctx: &Context, air: &Air, a: u32, d_trace_cols: *const u32, log_n: u32, d_mult: *mut u32) {
        ctx.check(air.with_raw(|ar| self.with_raw(|al| unsafe {
            smi_dev_xargs_multiplicities(ctx.raw, ar, al, a, d_trace_cols, self.n_cols, log_n, d_mult)
        })));
    }
    /// `smi_dev_xargs_columns` -> the mask of the arguments that close.
    pub fn columns(&self, ctx: &Context, air: &Air, d_trace_cols: *const u32, log_n: u32, challenges: &[u64; 8], d_c: *mut u32, c_stride: usize) -> u32 {
        let mut closes = 0u32;
        ctx.check(air.with_raw(|ar| self.with_raw(|al| unsafe {
            smi_dev_xargs_columns(ctx.raw, ar, al, d_trace_cols, self.n_cols, log_n, challenges.as_ptr(), d_c, c_stride, &mut closes)
        })));
        closes
    }
    /// `smi_dev_air_compose_xargs`: the composition plus the 2 A auxiliary quotients of this list.
    pub fn compose(&self, ctx: &Context, air: &Air, cfg: &smi_stark_cfg, d_lde: *const u32, stride: usize, d_c_lde: *const u32, c_stride: usize,
                   challenges: &[u64; 8], d_weights: *const u64, d_out: *mut u32, out_stride: usize) {
        ctx.check(air.with_raw(|ar| self.with_raw(|al| unsafe {
            smi_dev_air_compose_xargs(ctx.raw, cfg, ar, al, d_lde, stride, d_c_lde, c_stride, challenges.as_ptr(), d_weights, d_out, out_stride)
        })));
    }
    /// `smi_dev_air_prove_xargs` -> (root_1 then root_2, proof bytes, closes).
    pub fn prove(&self, ctx: &Context, air: &Air, cfg: &smi_stark_cfg, d_trace_cols: *const u32, grind_bits: u32) -> ([u8; 64], Vec<u8>, u32) {
        let mut roots = [0u8; 64];
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        let mut closes = 0u32;
        ctx.check(air.with_raw(|ar| self.with_raw(|al| unsafe {
            smi_dev_air_prove_xargs(ctx.raw, cfg, ar, al, d_trace_cols, roots.as_mut_ptr(), &mut proof, &mut len, std::ptr::null_mut(), std::ptr::null_mut(), grind_bits, &mut closes)
        })));
        let bytes = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { smi_free(proof as *mut c_void) };
        (roots, bytes, closes)
    }
    /// `smi_air_verify_xargs` -> `Ok(())` or the reason the proof is rejected.
    pub fn verify(&self, ctx: &Context, air: &Air, cfg: &smi_stark_cfg, roots: &[u8; 64], proof: &[u8], grind_bits: u32) -> Result<(), String> {
        let mut accept = 0 as c_int;
        ctx.check(air.with_raw(|ar| self.with_raw(|al| unsafe {
            smi_air_verify_xargs(ctx.raw, cfg, ar, al, roots.as_ptr(), proof.as_ptr(), proof.len(), &mut accept, grind_bits)
        })));
        if accept != 0 {
            Ok(())
        } else {
            Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned())
        }
    }
}

/// One lookup argument (include/stark_mi.h, "Lookup argument"): every row tuple over the `lookup` columns occurs among
/// the row tuples over the `table` columns, column `mult_col` holding the multiplicities; 1 ..= `SMI_LOOKUP_MAX_WIDTH`
/// columns a side, the lists may overlap, `mult_col` is none of them.
pub struct Lookup {
    lookup: Vec<u32>,
    table: Vec<u32>,
    mult_col: u32,
}

impl Lookup {
    pub fn new(lookup: &[u32], table: &[u32], mult_col: u32) -> Lookup {
        assert!(lookup.len() == table.len() && !lookup.is_empty() && lookup.len() <= SMI_LOOKUP_MAX_WIDTH as usize, "1 ..= SMI_LOOKUP_MAX_WIDTH columns a side");
        Lookup { lookup: lookup.to_vec(), table: table.to_vec(), mult_col }
    }
    fn with_raw<R>(&self, f: impl FnOnce(*const c_void) -> R) -> R {
        let raw = smi_air_lookup { width: self.lookup.len() as u32, mult_col: self.mult_col, lookup_col: self.lookup.as_ptr(), table_col: self.table.as_ptr() };
        f(&raw as *const smi_air_lookup as *const c_void)
    }
    /// `smi_dev_lookup_multiplicities`: the multiplicities of the device trace into `d_mult` (n residues, zeroed by the
    /// call) -> `Ok(())`, or the smallest row whose tuple is in no table row.
    pub fn multiplicities(&self, ctx: &Context, d_trace_cols: *const u32, n_cols: u32, log_n: u32, d_mult: *mut u32) -> Result<(), String> {
        let st = self.with_raw(|lk| unsafe { smi_dev_lookup_multiplicities(ctx.raw, lk, d_trace_cols, n_cols, log_n, d_mult) });
        if st == SMI_ERR_LOOKUP_MISSING {
            return Err(unsafe { CStr::from_ptr(smi_last_error(ctx.raw)) }.to_string_lossy().into_owned());
        }
        ctx.check(st);
        Ok(())
    }
    /// `smi_dev_lookup_column`: the column s of the device trace under the 8 unreduced challenges into four coordinate
    /// columns `s_stride` apart -> closes.  Panics with "no inverse" and the row when a denominator is zero.
    pub fn column(&self, ctx: &Context, d_trace_cols: *const u32, n_cols: u32, log_n: u32, challenges: &[u64; 8], d_s: *mut u32, s_stride: usize) -> bool {
        let mut closes = 0 as c_int;
        ctx.check(self.with_raw(|lk| unsafe {
            smi_dev_lookup_column(ctx.raw, lk, d_trace_cols, n_cols, log_n, challenges.as_ptr(), d_s, s_stride, &mut closes)
        }));
        closes != 0
    }
}

/// One permutation argument (include/stark_mi.h, "Permutation argument"): the multiset of the row tuples over the
/// `left` columns equals that over the `right` columns; 1 ..= `SMI_PERM_MAX_WIDTH` columns a side, the lists may overlap.
pub struct Permutation {
    left: Vec<u32>,
    right: Vec<u32>,
}

impl Permutation {
    pub fn new(left: &[u32], right: &[u32]) -> Permutation {
        assert!(left.len() == right.len() && !left.is_empty() && left.len() <= SMI_PERM_MAX_WIDTH as usize, "1 ..= SMI_PERM_MAX_WIDTH columns a side");
        Permutation { left: left.to_vec(), right: right.to_vec() }
    }
    fn with_raw<R>(&self, f: impl FnOnce(*const c_void) -> R) -> R {
        let raw = smi_air_perm { width: self.left.len() as u32, reserved0: 0, left_col: self.left.as_ptr(), right_col: self.right.as_ptr() };
        f(&raw as *const smi_air_perm as *const c_void)
    }
    /// `smi_dev_perm_column`: the column z of the device trace under the 8 unreduced challenges into four coordinate
    /// columns `z_stride` apart -> closes.  Panics with "no inverse" and the row when a denominator is zero.
    pub fn column(&self, ctx: &Context, d_trace_cols: *const u32, n_cols: u32, log_n: u32, challenges: &[u64; 8], d_z: *mut u32, z_stride: usize) -> bool {
        let mut closes = 0 as c_int;
        ctx.check(self.with_raw(|pm| unsafe {
            smi_dev_perm_column(ctx.raw, pm, d_trace_cols, n_cols, log_n, challenges.as_ptr(), d_z, z_stride, &mut closes)
        }));
        closes != 0
    }
}

/// `smi_grind_check` (host only): does `nonce` meet `bits` proof-of-work bits on `transcript`?
pub fn grind_check(transcript: &[u8], nonce: u64, bits: u32) -> bool {
    let mut ok = 0 as c_int;
    let st = unsafe { smi_grind_check(transcript.as_ptr(), transcript.len(), nonce, bits, &mut ok) };
    if st != SMI_OK {
        panic!("{}", status_text(st));
    }
    ok != 0
}

/// `smi_dev_grind`: the smallest nonce that meets `bits` proof-of-work bits on `transcript`, searched on the GPU below
/// `max_tries` (0: the default cap 2^(bits+6)); `None` when the cap is exhausted.
pub fn grind(ctx: &Context, transcript: &[u8], bits: u32, max_tries: u64) -> Option<u64> {
    let mut nonce = 0u64;
    let st = unsafe { smi_dev_grind(ctx.raw, transcript.as_ptr(), transcript.len(), bits, max_tries, &mut nonce) };
    if st == SMI_ERR_GRIND_EXHAUSTED {
        return None;
    }
    ctx.check(st);
    Some(nonce)
}
