/*
 * stark_mi.h -- C ABI of libstarkmi.so, the MI355X (gfx950) engine that stands behind
 * stark-rs's univariate / trace / fri / merkle API.
 *
 * The reference (0xSooki/stark-rs @ 2026-01-02) has no FFI of its own:
 * each entry point below names the Rust inherent method it replaces (file:line under
 * /root/reference) -- that method's body becomes a call to this function in the
 * binding shown in INTEGRATION.md.
 *
 * Conventions
 *   - Field values cross the boundary as contiguous little-endian u64, the reference's
 *     wire width (src/stream.rs:45, src/hash.rs:33).  They must be canonical (< p)
 *     unless a parameter says "unreduced ok" (SURVEY H6).
 *   - Digests are 32 raw bytes (src/hash.rs:1-2).
 *   - Every function returns an int32 status: 0 = ok, negative = the reference's panic
 *     (one code per message, smi_status_string gives the identical text so the Rust
 *     wrapper can `panic!` with it), <= -100 = HIP/runtime failure (smi_last_error).
 *   - No C++ exceptions, torch types or caller pointers retained across calls.
 *   - Functions named smi_dev_* take device pointers (u32 canonical residues, 4 B per
 *     element on device) and enqueue on the context's stream without synchronising.
 *     All others take host buffers and are synchronous on return.
 *   - A context is single-owner (not thread-safe), one per GPU / process.
 */
#ifndef STARK_MI_H
#define STARK_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: the reference's panic messages ------------------------------- */
enum {
    SMI_OK = 0,
    SMI_ERR_NO_INVERSE = -1,          /* "no inverse"                         src/ff.rs:171 */
    SMI_ERR_DIV_BY_ZERO = -2,         /* "no division by zero"                src/ff.rs:182 */
    SMI_ERR_NOT_POW2 = -3,            /* "n must be a power of two"           src/ff.rs:217 */
    SMI_ERR_ROOT_TOO_LARGE = -4,      /* "n > 2^23 not supported by this modulus" src/ff.rs:218 */
    SMI_ERR_EMPTY_LEAVES = -5,        /* "Cannot create tree from empty leaves"   src/merkle.rs:12 */
    SMI_ERR_LEAVES_NOT_POW2 = -6,     /* "Number of leaves must be power of 2"    src/merkle.rs:13-16 */
    SMI_ERR_INDEX_OOB = -7,           /* "Index out of bounds"                src/merkle.rs:68 */
    SMI_ERR_DOMAIN_NOT_POW2 = -8,     /* "Domain length must be power of 2"   src/fri.rs:37-40 */
    SMI_ERR_EXPANSION_NOT_POW2 = -9,  /* "Expansion factor must be power of 2" src/fri.rs:41-44 */
    SMI_ERR_EXPANSION_TOO_SMALL = -10,/* "Expansion factor must be at least 4" src/fri.rs:45 */
    SMI_ERR_CODEWORD_LEN = -11,       /* "initial codeword length does not match domain length" src/fri.rs:256-260 */
    SMI_ERR_SAMPLE_ENTROPY = -12,     /* "not enough entropy in indices wrt last codeword" src/fri.rs:183-186 */
    SMI_ERR_SAMPLE_TOO_MANY = -13,    /* "cannot sample more indices than available in last codeword" src/fri.rs:187-192 */
    SMI_ERR_LEN_MISMATCH = -14,       /* assert!(domain.len() == values.len()) src/univariate/interpolate.rs:10 */
    SMI_ERR_EMPTY_DOMAIN = -15,       /* assert!(domain.len() > 0)            src/univariate/interpolate.rs:11 */
    SMI_ERR_WRONG_FIELD = -16,        /* assert!(self.p == 998244353)         src/ff.rs:192,216 */
    SMI_ERR_POLY_DIV_BY_ZERO = -18,   /* "No division by zero"                src/univariate/div.rs:7-9 */
    SMI_ERR_NO_ROUNDS = -17,          /* num_rounds()==0: proof the reference's verify rejects */
    /* contract violations that have no reference counterpart */
    SMI_ERR_BAD_ARG = -50,
    SMI_ERR_NON_CANONICAL = -51,      /* a field value >= p where the precondition forbids it (H6) */
    SMI_ERR_UNSUPPORTED_PRIME = -52,  /* p must be an odd prime < 2^30 with p-1 divisible by the sizes used */
    SMI_ERR_NOT_GEOMETRIC = -53,      /* domain is not offset*omega^k: caller must fall back to the CPU code */
    SMI_ERR_COLUMNS_NOT_BOUND = -54,  /* smi_stark_verify on a proof made without open_columns: nothing in it refers to the
                                         column roots, so it can only be checked as a FRI proof (smi_fri_verify) */
    SMI_ERR_GRIND_EXHAUSTED = -55,    /* no nonce below the search cap meets the proof-of-work difficulty ("Grinding") */
    SMI_ERR_LOOKUP_MISSING = -56,     /* smi_dev_lookup_multiplicities: a looked-up tuple is in no table row ("Lookup argument") */
    /* runtime */
    SMI_ERR_HIP = -100,
    SMI_ERR_NO_DEVICE = -101,
    SMI_ERR_OOM = -102,
    SMI_ERR_RCCL = -103               /* RCCL (or the caller's collective shim) failed: smi_last_error */
};

typedef struct smi_ctx smi_ctx;
typedef struct smi_tree smi_tree;     /* device-resident MerkleTree (all levels) */
typedef struct smi_fri_run smi_fri_run; /* device-resident artefacts of one Fri::commit */

const char *smi_status_string(int status);
const char *smi_last_error(const smi_ctx *ctx);
const char *smi_version(void);

/* ---- context -------------------------------------------------------------------- */
/* FiniteField::new(p) (src/ff.rs:109-111) plus the generator g() (src/ff.rs:191-197):
 * (998244353, 3) is the reference field; (469762049, 3) is the build's second prime
 * for domains above 2^23.  device = HIP device ordinal. */
int smi_ctx_create(uint64_t p, uint64_t g, int device, smi_ctx **out);
void smi_ctx_destroy(smi_ctx *ctx);
/* Use an existing hipStream_t (e.g. torch's current stream) for everything enqueued. */
int smi_ctx_set_stream(smi_ctx *ctx, void *hip_stream);
int smi_ctx_sync(smi_ctx *ctx);
/* Per-kernel timing with HIP events on the context's stream (bench.py's roofline leg):
 * while enabled, every hot-path kernel launch is bracketed by two events.
 * smi_ctx_profile_read synchronises, aggregates by kernel name and clears the log. */
typedef struct {
    char name[56];
    uint32_t launches;
    double total_ms;
    double alg_bytes;   /* algorithmic bytes summed over the launches (DESIGN.md states the per-unit figures) */
    double alg_mixes;   /* hash kernels: mix_state evaluations (src/hash.rs:59-86) the launches' leaf and node hashes
                           amount to -- 9 per 8-byte leaf, 10 per node (src/hash.rs:14-27,41-46); 0 elsewhere */
} smi_kernel_time;
int smi_ctx_profile(smi_ctx *ctx, int enable);
int smi_ctx_profile_read(smi_ctx *ctx, smi_kernel_time *out, size_t cap, size_t *n);
/* Restrict the brackets to launches whose kernel name contains name_part (NULL or "": all launches).  Bracketing every
 * launch perturbs what it measures -- kernels no longer run back to back and the chip clocks higher -- so bench.py
 * times its dominant kernel with only that kernel bracketed, inside an otherwise undisturbed loop. */
int smi_ctx_profile_only(smi_ctx *ctx, const char *name_part);
/* Measurement aid for the roofline leg: while enabled, every NTT pass launches its copy-only twin
 * (same tiles, same global loads and store addresses, no arithmetic) so that smi_ctx_profile
 * times what HBM delivers for each pass's access pattern.  Outputs are meaningless while it is
 * on; never enable it in product use. */
int smi_ctx_copy_probe(smi_ctx *ctx, int enable);
/* Measurement aid for the prove's roofline (bench.py `prove_roofline`): the hash's permutation and nothing else --
 * `mixes` back-to-back mix_state evaluations (src/hash.rs:59-86) per hash, two hashes per lane in the layout the
 * Merkle kernels use, enough workgroups to fill the chip, no memory traffic -- timed with HIP events on the
 * context's stream.  *mixes_per_s is the integer-VALU ceiling of this formulation of the hash on this GPU, at the
 * clock the chip sustains under that load; the Merkle kernels are reported against it. */
int smi_ctx_mix_probe(smi_ctx *ctx, uint32_t mixes, double *mixes_per_s);
/* smi_dev_lde / smi_lde at 2^20..2^22 rows: run the extension in two passes over its outputs (coset-split
 * pass A, interleaving pass B -- csrc/lde_core.h) instead of the generic three.  Same results; off by
 * default (within 2 % of the generic path on MI355X); SMI_LDE_TWO_PASS=1 sets the default. */
int smi_ctx_lde_two_pass(smi_ctx *ctx, int enable);
uint64_t smi_ctx_modulus(const smi_ctx *ctx);
uint32_t smi_ctx_two_adicity(const smi_ctx *ctx);

/* ---- field scalars (host, exact restatements needed by callers) ------------------ */
/* FiniteField::prim_nth_root (src/ff.rs:215-223): g^((p-1)/n). */
int smi_prim_nth_root(const smi_ctx *ctx, uint64_t n, uint64_t *out);
/* FiniteField::inv via Fermat; SMI_ERR_NO_INVERSE for 0 (src/ff.rs:169-178). */
int smi_ff_inv(const smi_ctx *ctx, uint64_t x, uint64_t *out);
int smi_ff_exp(const smi_ctx *ctx, uint64_t base, uint64_t e, uint64_t *out); /* src/ff.rs:200-213 */
int smi_ff_mul(const smi_ctx *ctx, uint64_t a, uint64_t b, uint64_t *out);    /* src/ff.rs:138-144 */

/* ---- univariate: host-buffer entry points ---------------------------------------- */
/* Polynomial::interpolate_domain (src/univariate/interpolate.rs:6-44) for the geometric
 * domain d[k] = offset * omega_n^k, n = 2^log_n, omega_n = prim_nth_root(n):
 * coeffs[j] = offset^-j n^-1 sum_k values[k] omega_n^-jk.  Always writes n coefficients
 * (trailing zeros included); Polynomial equality ignores them (src/univariate/mod.rs:13-39). */
int smi_intt(smi_ctx *ctx, const uint64_t *values, uint64_t *coeffs, uint32_t log_n, uint64_t offset);
/* Polynomial::eval_domain (src/univariate/eval.rs:16-21) on d[k] = offset * omega_N^k,
 * N = 2^log_N, n_coeffs <= N: evals[k] = sum_j coeffs[j] d[k]^j, in domain order. */
int smi_coset_ntt(smi_ctx *ctx, const uint64_t *coeffs, size_t n_coeffs, uint64_t *evals, uint32_t log_N,
                  uint64_t offset);
/* Polynomial::scale (src/univariate/mod.rs:99-113): out[i] = coeffs[i] * factor^i. */
int smi_poly_scale(smi_ctx *ctx, const uint64_t *coeffs, size_t n, uint64_t factor, uint64_t *out);
/* Polynomial::mul (src/univariate/mul.rs:6-29) by NTT: out gets na+nb-1 coefficients (*n_out),
 * or *n_out = 0 when either operand is the zero polynomial, as the reference returns `vec![]`. */
int smi_poly_mul(smi_ctx *ctx, const uint64_t *a, size_t na, const uint64_t *b, size_t nb, uint64_t *out, size_t *n_out);
/* Polynomial::div (src/univariate/div.rs:6-42): quotient and remainder of a / b, via the power-series
 * inverse of the reversed divisor (NTT products) instead of the reference's O(n*m) subtraction loop.
 * q gets deg a - deg b + 1 coefficients (*nq), r gets deg b coefficients (*nr; the reference's
 * remainder vector may carry further trailing zeros -- Polynomial equality ignores them).  When
 * deg a < deg b: *nq = 0 and r = a unchanged (na coefficients), as div.rs:10-18.  A zero divisor
 * gives SMI_ERR_POLY_DIV_BY_ZERO.  q needs room for na, r for max(na, nb) coefficients. */
int smi_poly_div(smi_ctx *ctx, const uint64_t *a, size_t na, const uint64_t *b, size_t nb, uint64_t *q, size_t *nq, uint64_t *r,
                 size_t *nr);
/* Checks in O(n) whether domain[k] == domain[0]*omega_n^k (the fast-path contract of
 * interpolate_domain / eval_domain); returns SMI_OK and *offset = domain[0], or
 * SMI_ERR_NOT_GEOMETRIC. */
int smi_domain_is_geometric(const smi_ctx *ctx, const uint64_t *domain, size_t n, uint64_t *offset);

/* ---- univariate on arbitrary points: subproduct trees on the device (batched NTT products, LDS blocks of 256 points
 * at the bottom; the number of launches grows with log n).  Points need not be geometric -- callers with a domain
 * offset*omega^k keep smi_intt / smi_coset_ntt.  A value >= p gives SMI_ERR_NON_CANONICAL.  K is the modulus'
 * usable two-adicity (smi_ctx_two_adicity: 23 for 998244353, 26 for 469762049); larger calls give
 * SMI_ERR_ROOT_TOO_LARGE. */
/* Polynomial::zerofier (src/univariate/mod.rs:77-96): prod_i (x - domain[i]); writes n+1 coefficients, monic.
 * Duplicates and 0 are allowed.  n == 0 -> SMI_ERR_EMPTY_DOMAIN (the reference indexes domain[0]).
 * n <= 2^K: 2^23 points on 998244353, 2^26 on 469762049. */
int smi_poly_zerofier(smi_ctx *ctx, const uint64_t *domain, size_t n, uint64_t *coeffs);
/* Polynomial::eval_domain (src/univariate/eval.rs:16-21) on ANY point list: values[k] = f(points[k]), in order.
 * n_coeffs and n_points are independent (either may be 0; n_coeffs > n_points is allowed); duplicates allowed.
 * max(n_coeffs, n_points) <= 2^(K-1): the root's power-series products take one doubling more than the tree
 * (2^22 on 998244353, 2^25 on 469762049). */
int smi_poly_eval_points(smi_ctx *ctx, const uint64_t *coeffs, size_t n_coeffs, const uint64_t *points, size_t n_points,
                         uint64_t *values);
/* Polynomial::interpolate_domain (src/univariate/interpolate.rs:6-44) on ANY domain of distinct points: writes n
 * coefficients (trailing zeros included, same contract as smi_intt).  A repeated point -> SMI_ERR_NO_INVERSE
 * "no inverse" (the reference's field.inv panic, interpolate.rs:34); n == 0 -> SMI_ERR_EMPTY_DOMAIN.
 * n <= 2^(K-1), as smi_poly_eval_points (2^22 on 998244353, 2^25 on 469762049). */
int smi_poly_interpolate_points(smi_ctx *ctx, const uint64_t *domain, const uint64_t *values, size_t n, uint64_t *coeffs);

/* ---- trace: Trace::get_col / to_field_elements (src/trace.rs:21-34) --------------- */
/* Low-degree extension of a column-major trace: for each of n_cols columns (n = 2^log_n
 * values on the subgroup domain trace_offset*omega_n^k) interpolate, then evaluate on
 * lde_offset*omega_N^k, N = n << log_blowup.  out is column-major n_cols x N. */
int smi_lde(smi_ctx *ctx, const uint64_t *cols, uint32_t n_cols, uint32_t log_n, uint32_t log_blowup,
            uint64_t trace_offset, uint64_t lde_offset, uint64_t *out);
/* Row-major i128 trace (src/trace.rs:4-7, each value as 16 LE bytes) -> column-major u64,
 * `e as u64` then reduced mod p for the device (precondition H6 made explicit). */
int smi_trace_pack(const smi_ctx *ctx, const void *rows_i128, size_t n_rows, size_t n_cols, uint64_t *cols_out);

/* ---- hash / merkle ---------------------------------------------------------------- */
/* Hash::from_field_elements(&[e]) for each e (src/hash.rs:32-35 as used at src/fri.rs:118-121):
 * digests gets n x 32 bytes. */
int smi_hash_leaves(smi_ctx *ctx, const uint64_t *elems, size_t n, uint8_t *digests);
/* Hash::combine (src/hash.rs:41-46) for n pairs: out[i] = H(left_right[2i] || left_right[2i+1]). */
int smi_hash_combine_pairs(smi_ctx *ctx, const uint8_t *digests, size_t n_pairs, uint8_t *out);
/* Hash::from_bytes (src/hash.rs:7-30) of one message (device single-lane kernel). */
int smi_hash_bytes(smi_ctx *ctx, const uint8_t *msg, size_t len, uint8_t out[32]);
/* The same for n messages of msg_len bytes each (msgs: n x msg_len, out: n x 32), one device lane
 * per message: Fri::sample_indices hashes seed || counter for a run of counters (src/fri.rs:176-213). */
int smi_hash_bytes_batch(smi_ctx *ctx, const uint8_t *msgs, size_t n, size_t msg_len, uint8_t *out);
/* MerkleTree::commit (src/merkle.rs:44-65). */
int smi_merkle_commit(smi_ctx *ctx, const uint8_t *leaves, size_t n, uint8_t root[32]);
/* MerkleTree::new (src/merkle.rs:11-38); the tree (all levels) stays on the device. */
int smi_merkle_new(smi_ctx *ctx, const uint8_t *leaves, size_t n, smi_tree **out);
/* Fused leaf hashing + tree over a codeword, one element per leaf (src/fri.rs:118-127). */
int smi_merkle_from_codeword(smi_ctx *ctx, const uint64_t *codeword, size_t n, smi_tree **out);
int smi_merkle_root(smi_ctx *ctx, const smi_tree *t, uint8_t root[32]);          /* get_root, src/merkle.rs:40-42 */
/* MerkleTree::open (src/merkle.rs:67-80): path gets *depth = log2(n) digests. */
int smi_merkle_open(smi_ctx *ctx, const smi_tree *t, size_t index, uint8_t *path, size_t *depth);
/* Copies level `level` (0 = leaves) to the host: nodes[level] of src/merkle.rs:6. */
int smi_merkle_level(smi_ctx *ctx, const smi_tree *t, uint32_t level, uint8_t *out, size_t *n_out);
/* MerkleTree::verify (src/merkle.rs:82-96) for k (leaf, index, path) triples that share one depth
 * and one root -- the verifier's hot loop (src/fri.rs:464-497); ok[i] = 1 if path i authenticates. */
int smi_merkle_verify_batch(smi_ctx *ctx, const uint8_t *leaves, const uint64_t *indices, const uint8_t *paths, size_t k,
                            size_t depth, const uint8_t root[32], uint8_t *ok);
size_t smi_merkle_num_leaves(const smi_tree *t);
void smi_merkle_free(smi_tree *t);

/* ---- fri --------------------------------------------------------------------------- */
/* Fri::new's fields (src/fri.rs:8-15,30-55). */
typedef struct {
    uint64_t omega;
    uint64_t offset;
    uint64_t domain_length;
    uint64_t expansion_factor;
    uint64_t num_colinearity_tests;
} smi_fri_cfg;

int smi_fri_check(const smi_ctx *ctx, const smi_fri_cfg *cfg);                   /* asserts of src/fri.rs:37-45 */
int smi_fri_num_rounds(const smi_fri_cfg *cfg, uint64_t *rounds);                /* src/fri.rs:93-103 */
/* Fri::fold_codeword (src/fri.rs:57-91); alpha may be an unreduced u64 (src/fiat_shamir.rs:23-24). */
int smi_fri_fold(smi_ctx *ctx, const uint64_t *codeword, size_t len, uint64_t alpha, uint64_t offset,
                 uint64_t omega, uint64_t *out);
/* Fri::commit (src/fri.rs:105-156) with a fresh FiatShamir: roots gets R x 32 bytes, alphas
 * R-1 unreduced challenges, last_codeword domain_length >> (R-1) values.  *run (optional)
 * keeps every round's codeword and tree on the device (smi_fri_run_* accessors below). */
int smi_fri_commit(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint64_t *codeword, size_t len, uint8_t *roots,
                   uint64_t *alphas, uint64_t *last_codeword, size_t *last_len, smi_fri_run **run);
/* Fri::commit (src/fri.rs:105-156) with the caller's `&mut FiatShamir`: transcript / transcript_len are the bytes its
 * `transcript` holds before the call (host memory; NULL with 0 is a fresh FiatShamir, NULL with a length is
 * SMI_ERR_BAD_ARG).  Each root is absorbed after them (src/fri.rs:131) and every challenge hashes the whole transcript
 * (src/fiat_shamir.rs:19-25).  The roots are what Fri::commit pushes after the caller's objects; the transcript itself
 * is not written: the caller appends the R roots to it, as the reference leaves it.  Outputs as smi_fri_commit. */
int smi_fri_commit_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint64_t *codeword,
                      size_t len, uint8_t *roots, uint64_t *alphas, uint64_t *last_codeword, size_t *last_len, smi_fri_run **run);
/* Fri::prove (src/fri.rs:250-311) with a fresh FiatShamir and ProofStream, returning
 * ProofStream::serialize (src/stream.rs:35-64).  *proof is malloc'd: release with smi_free.
 * top_indices gets num_colinearity_tests entries (the method's return value). */
int smi_fri_prove(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint64_t *codeword, size_t len, uint8_t **proof,
                  size_t *proof_len, uint64_t *top_indices);
/* Fri::prove (src/fri.rs:250-311) with the caller's `&mut FiatShamir` and `&mut ProofStream`: transcript as in
 * smi_fri_commit_fs (host memory).  *proof is the serialization of the objects Fri::prove pushes AFTER the caller's
 * own (the caller's stream is unchanged by them); the caller then absorbs the R roots, as the reference leaves its
 * transcript.  Outputs as smi_fri_prove. */
int smi_fri_prove_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint64_t *codeword,
                     size_t len, uint8_t **proof, size_t *proof_len, uint64_t *top_indices);
/* The `codewords` Fri::commit returns (src/fri.rs:153-155): their count, one of them (out may be
 * NULL to query *len), and MerkleTree::open on a round's retained tree. */
/* Fri::verify (src/fri.rs:313-504) of a serialized ProofStream against a fresh FiatShamir: *accept = 1 where the
 * reference returns true, 0 where it prints a reason and returns false (smi_last_error has the reason); a
 * reference panic (e.g. a last codeword whose length is not a power of two, src/merkle.rs:13-16) is that panic's
 * status.  pv_indices / pv_values (optional, 2*t entries each) receive the (index, value) pairs the reference
 * pushes to polynomial_values.  Leaf hashes and authentication paths are checked in device batches, the last
 * layer's degree by an inverse + forward NTT; SMI_ERR_NOT_GEOMETRIC if cfg's omega does not generate the domain.
 * Two deliberate differences from the reference on malformed proofs, both failing closed (a status, never accept):
 *   - a last codeword whose length is not domain_length >> (rounds - 1) but whose Merkle root matches: the reference
 *     runs its O(L^3) Lagrange interpolation over the (then repeating or truncated) point list and returns whatever
 *     that gives or panics with "no inverse"; the NTT needs the points to be a whole coset, so this returns
 *     SMI_ERR_NOT_GEOMETRIC;
 *   - unreduced values (>= p) in a triple: the colinearity test uses the reference's own `(p + l - r) % p` in u128
 *     (src/ff.rs:154-160) including its release-build wrap for r > p + l (a debug build of the reference panics
 *     there), and the leaf is hashed from the raw u64, as in the reference. */
int smi_fri_verify(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *proof, size_t proof_len, int *accept, uint64_t *pv_indices,
                   uint64_t *pv_values, size_t *n_pv);
/* Fri::verify (src/fri.rs:313-504) with the caller's `&mut FiatShamir` (transcript as in smi_fri_commit_fs, host memory)
 * and `&mut ProofStream`: proof holds the objects still to be popped, starting with the ones Fri::prove pushed after
 * the caller's objects.  *accept, pv_indices / pv_values / n_pv as in smi_fri_verify.  *consumed (optional): on
 * acceptance the bytes of the objects Fri::verify popped, so a caller whose stream carries more objects goes on from
 * proof + *consumed; 0 on rejection.  The caller absorbs the R roots, as the reference leaves its transcript. */
int smi_fri_verify_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                      size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed);
int smi_fri_run_num_codewords(const smi_fri_run *run, size_t *n);
int smi_fri_run_codeword(smi_fri_run *run, size_t round, uint64_t *out, size_t *len);
int smi_fri_run_open(smi_fri_run *run, size_t round, size_t index, uint8_t *path, size_t *depth);
void smi_fri_run_free(smi_fri_run *run);
void smi_free(void *p);

/* ---- device-resident entry points (u32 residues, context stream, no sync) ---------- */
int smi_dev_alloc(smi_ctx *ctx, size_t bytes, void **d_ptr);
int smi_dev_free(smi_ctx *ctx, void *d_ptr);
/* u64 host -> u32 device (checks canonical unless reduce != 0) and back. */
int smi_dev_upload_u64(smi_ctx *ctx, const uint64_t *host, size_t n, uint32_t *d_out, int reduce);
int smi_dev_download_u64(smi_ctx *ctx, const uint32_t *d_in, size_t n, uint64_t *host);

/* Batched NTT kernel driver.  For each of `batch` columns (column c at d_in + c*in_stride,
 * d_out + c*out_stride, strides in elements):
 *   inverse == 0: out[k] = sum_{j<n_in} in[j] (offset*omega_N^k)^j        (coset NTT, zero-padded)
 *   inverse != 0: out[j] = scale * offset^-j N^-1 sum_k in[k] omega_N^-jk (n_in must equal N)
 * N = 2^log_n; natural order in and out; d_in may equal d_out (columns must not overlap).
 * post_scale (canonical, 1 = none) multiplies every output of the inverse transform by
 * post_scale^j -- the fused `Polynomial::scale` (src/univariate/mod.rs:99-113) of an LDE. */
int smi_dev_ntt(smi_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, uint32_t log_n, size_t n_in, uint32_t batch,
                size_t in_stride, size_t out_stride, int inverse, uint64_t offset, uint64_t post_scale);
/* LDE of a column-major device trace: d_out is n_cols x (n << log_blowup), stride N. */
int smi_dev_lde(smi_ctx *ctx, const uint32_t *d_cols, uint32_t n_cols, uint32_t log_n, uint32_t log_blowup,
                uint64_t trace_offset, uint64_t lde_offset, uint32_t *d_out);
/* Leaf digests only / fused leaf hashing + all tree levels.  d_nodes: (2n-1) x 32 bytes,
 * level 0 (leaf digests) first, root last -- `nodes` of src/merkle.rs:18-33 back to back. */
int smi_dev_hash_leaves(smi_ctx *ctx, const uint32_t *d_elems, size_t n, uint8_t *d_digests);
int smi_dev_merkle_build(smi_ctx *ctx, const uint32_t *d_elems, size_t n, uint8_t *d_nodes);
/* Row-leaf tree (build-defined leaf rule): leaf i = Hash::from_field_elements of row i
 * of n_cols columns (column c at d_cols + c*col_stride), i.e. src/hash.rs:32-35 applied to the row
 * instead of to a single element; with 4 columns a leaf is one 32-byte chunk and costs what a
 * single-element leaf costs, so one tree replaces four. */
int smi_dev_merkle_build_rows(smi_ctx *ctx, const uint32_t *d_cols, uint32_t n_cols, size_t col_stride, size_t n, uint8_t *d_nodes);
/* Coset-leaf tree: a group of n_cols (1 .. 64) columns of n residues, n a power of two and at least 4, column c at
 * d_cols + c*col_stride with col_stride >= n.  With q = n / 4, leaf i < q = Hash::from_field_elements of 4 n_cols values,
 * value 4 c + j = column c at index i + j q, j = 0 .. 3: one leaf per coset {i, i + q, i + 2 q, i + 3 q} of a fold by 4,
 * in the order of fold-by-4 FRI's leaf (coordinate outer, coset point inner), so a four-coordinate codeword's tree
 * here is the tree of "Extension FRI, folding factor 4" and a trace tree follows the same rule.  One opening then
 * serves all four points: one leaf and log2 q digests.  d_nodes: (2 q - 1) x 32 bytes, levels as above; q = 1 is a tree
 * of one digest.  SMI_ERR_BAD_ARG (smi_last_error has the sentence) when n is not a power of two or n < 4, when
 * col_stride < n, or when n_cols is outside 1 .. 64. */
int smi_dev_merkle_build_cosets(smi_ctx *ctx, const uint32_t *d_cols, uint32_t n_cols, size_t col_stride, size_t n, uint8_t *d_nodes);
/* Tree over precomputed 32-byte leaves already at d_nodes[0 .. n*32). */
int smi_dev_merkle_from_digests(smi_ctx *ctx, size_t n, uint8_t *d_nodes);
/* Hash::from_bytes (src/hash.rs:7-30) of a message in device memory, digest to device memory: a
 * transcript that lives on the device (roots in, the challenge = first 8 digest bytes out, see
 * src/fiat_shamir.rs:19-25) needs no host round trip per round. */
int smi_dev_hash_bytes(smi_ctx *ctx, const uint8_t *d_msg, size_t len, uint8_t *d_out32);
/* Fri::fold_codeword with alpha read from device memory (*d_alpha: one unreduced u64). */
int smi_dev_fri_fold(smi_ctx *ctx, const uint32_t *d_in, size_t len, const uint64_t *d_alpha, uint64_t offset,
                     uint64_t omega, uint32_t *d_out);
/* The same fold for one shard of a codeword distributed over several GPUs: `count`
 * outputs starting at global output index index0, d_lo[k] = c[index0+k], d_hi[k] =
 * c[index0+k+full_len/2] (the second operand arrives from the partner GPU). */
int smi_dev_fri_fold_shard(smi_ctx *ctx, const uint32_t *d_lo, const uint32_t *d_hi, size_t count, size_t index0,
                           size_t full_len, const uint64_t *d_alpha, uint64_t offset, uint64_t omega, uint32_t *d_out);
/* Fri::commit + the query phase of Fri::prove over a device codeword.  Roots, alphas and
 * the serialized proof are produced without a host round trip per round: Fiat-Shamir and
 * index sampling run in single-lane device kernels. */
int smi_dev_fri_prove(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint32_t *d_codeword, size_t len, uint8_t **proof,
                      size_t *proof_len, uint64_t *top_indices, smi_fri_run **run);
/* smi_dev_fri_prove continuing the caller's FiatShamir (Fri::prove, src/fri.rs:250-311, as smi_fri_prove_fs): the
 * transcript is a HOST pointer (the reference's transcript is a host Vec<u8>; its state is computed on the host and
 * passed to the first launch by value).  The proof is what Fri::prove pushes after the caller's objects. */
int smi_dev_fri_prove_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_codeword,
                         size_t len, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, smi_fri_run **run);

/* out[i] = sum_c (weights[c] mod p) * cols[c*stride + i]; d_weights holds n_cols unreduced u64
 * challenges on the device (random linear combination of committed columns; build-defined,
 * the reference has no prover above Fri::prove -- SURVEY F5). */
int smi_dev_combine_columns(smi_ctx *ctx, const uint32_t *d_cols, uint32_t n_cols, size_t len, size_t stride,
                            const uint64_t *d_weights, uint32_t *d_out);
/* Build-defined composition of the reference primitives: column-major device
 * trace -> LDE (blowup 2^log_blowup on the coset lde_offset*<w_N>) -> one Merkle tree per column
 * (one element per leaf, src/fri.rs:118-121) -> fresh FiatShamir absorbs the column roots and
 * draws one weight per column -> Fri::prove (src/fri.rs:250-311, expansion_factor = blowup) on
 * the weighted sum.  column_roots (host, optional) gets n_cols x 32 bytes; *proof is the
 * serialized FRI ProofStream (smi_free); stage_ms (optional) gets the HIP-event times of
 * {lde, column commits, combine, fri} in milliseconds. */
typedef struct {
    uint32_t log_n, log_blowup, n_cols;
    uint32_t row_leaves;   /* 0: one tree per column, one element per leaf (the reference's leaf rule, src/fri.rs:118-121);
                              1: one tree over the rows (smi_dev_merkle_build_rows) -- a build-defined variant */
    uint64_t trace_offset, lde_offset, num_colinearity_tests;
    uint64_t open_columns; /* 1: after the FRI objects, bind the combined codeword to the committed columns -- for every
                              colinearity test s, with a = top_index[s] mod N/2 and b = a + N/2 (the layer-0 positions
                              Fri::query opens, src/fri.rs:215-248): FieldElements([col_0[a] .. col_{W-1}[a]]),
                              FieldElements([col_0[b] .. col_{W-1}[b]]) for s = 0 .. t-1, then MerklePath(col_c, a),
                              MerklePath(col_c, b) for every s and, inside it, every c (tags and widths of src/stream.rs:35-64).  A verifier checks each path against
                              column root c and sum_c weight_c * col_c[a] against the FRI triple's value.  Column trees only. */
} smi_stark_cfg;
int smi_dev_stark_prove(smi_ctx *ctx, const smi_stark_cfg *cfg, const uint32_t *d_trace_cols, uint8_t *column_roots,
                        uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms);

/* Verifier of smi_dev_stark_prove / smi_mgpu_stark_prove (column trees, cfg->open_columns != 0): Fri::verify of the
 * leading objects on the domain lde_offset * <w_N>, then the column openings -- every authentication path against
 * its column root (column_roots: n_cols x 32) and sum_c weight_c * col_c[a] against the layer-0 triple -- with
 * the weights re-derived from the column roots.  *accept as in smi_fri_verify.  A proof made with open_columns == 0
 * is exactly Fri::prove's bytes: no object in it refers to the column roots, so accepting it here would present a
 * low-degree proof of an unrelated codeword as a proof about these columns.  The call therefore returns
 * SMI_ERR_COLUMNS_NOT_BOUND (*accept = 0, nothing verified) when cfg->open_columns == 0; check such a proof
 * with smi_fri_verify. */
int smi_stark_verify(smi_ctx *ctx, const smi_stark_cfg *cfg, const uint8_t *column_roots, const uint8_t *proof, size_t proof_len,
                     int *accept);

/* ---- AIR: boundary and transition constraints over the committed columns --------------------
 * The reference stops at Fri (its Trace has a constructor and no consumer); its naming follows the
 * "Anatomy of a STARK" construction, whose next step this is: a proof that the W committed columns satisfy
 * boundary constraints (column c holds value v in row r) and transition constraints (polynomials in the cells of
 * two consecutive rows that vanish on every row pair (r, r+1), r = 0 .. n-2, no wrap-around).
 *
 * Flat, pointer-plus-count, host memory.  Transition constraint k is
 *   C_k(X_0 .. X_{2W+2Q-1}) = sum_{terms of k} coeff * prod_{factors} X_var^exp,
 * with four kinds of variable (W = n_cols, Q = n_periodic):
 *   var = c           (c < W)   trace column c at this row;        var = W + c        trace column c at the next row;
 *   var = 2W + j      (j < Q)   periodic column j at this row;     var = 2W + Q + j   periodic column j at the next row.
 * Its degree d_k is the largest sum of exponents over its terms, periodic factors counted like trace factors,
 * d = max(1, max_k d_k), D = the smallest power of two >= max(1, d-1), E = 2^log_blowup / D: the expansion factor
 * FRI runs at (the quotients have degree < D * n).
 *
 * Periodic columns (round constants, selectors, public columns).  Column j has a period P_j = 2^l_j, 0 <= l_j <= log_n,
 * and P_j canonical values v_j[0 .. P_j); row r holds v_j[r mod P_j].  P_j = 1 is a constant, P_j = n a fully public
 * column.  They are part of the statement, like the coefficients and the boundary values: prover and verifier both
 * hold them, and they are not committed, not opened, carry no weight and do not enter the transcript -- the proof
 * bytes of an AIR with periodic columns have the layout of one without.  As a polynomial, column j is pi_j, the
 * unique one of degree < n with pi_j(tau w^r) = v_j[r mod P_j]; X_{2W+j} = pi_j(x) and X_{2W+Q+j} = pi_j(w x).
 * pi_j(x) = q_j((x / tau)^(n / P_j)) with q_j the interpolant of v_j on the P_j-th roots of unity, so on the evaluation
 * coset pi_j(x_i) depends on i mod (P_j * B) only: the library extends v_j to P_j * B values with smi_dev_lde
 * (log_n = l_j, trace_offset 1, lde_offset (h / tau)^(n / P_j)) and the kernels read that table modulo its length.
 * On the trace itself (smi_dev_air_check) the operands of row pair (r, r+1) are v_j[r mod P_j] and v_j[(r+1) mod P_j].
 *
 * The composition codeword.  p the modulus, n = 2^log_n, B = 2^log_blowup, N = nB, w = omega_n, tau = trace_offset,
 * h = lde_offset, x_i = h * omega_N^i, lde[c][i] = f_c(x_i) (smi_dev_lde, natural order; the next row is the index
 * shift f_c(w x_i) = lde[c][(i + B) mod N]).
 *   column c with boundary points {(r_j, v_j)}: I_c the interpolant through (tau w^r_j, v_j), Z_c(x) = prod_j (x - tau w^r_j),
 *       term_c(x_i) = (lde[c][i] - I_c(x_i)) / Z_c(x_i);   without boundary points term_c(x_i) = lde[c][i];
 *   tq_k(x_i) = C_k(lde[.][i], lde[.][(i+B) mod N], pi_.(x_i), pi_.(w x_i)) * (x_i - tau w^(n-1)) / (x_i^n - tau^n);
 *   cw[i] = sum_{c<W} (weight_c mod p) * term_c(x_i) + sum_{k<K} (weight_{W+k} mod p) * tq_k(x_i)   (mod p).
 * With K = 0 and no boundary point this is smi_dev_combine_columns.
 *
 * Limits (SMI_ERR_BAD_ARG, the text of smi_air_last_error / smi_last_error names the one that was broken):
 *   n_cols <= 64; n_constraints <= SMI_AIR_MAX_CONSTRAINTS; n_terms <= SMI_AIR_MAX_TERMS; at most
 *   SMI_AIR_MAX_TERM_FACTORS factors in a term; 1 <= factor_exp <= SMI_AIR_MAX_EXP; factor_var < 2 * n_cols +
 *   2 * n_periodic; at most SMI_AIR_MAX_BOUNDARY_PER_COL boundary points in a column, a (col, row) pair at most once,
 *   row < n; n_periodic <= SMI_AIR_MAX_PERIODIC; periodic_log_period[j] <= log_n;
 *   offsets in 1 .. p-1.  Refused as well (SMI_ERR_BAD_ARG): lde_offset^N == 1, and (lde_offset / trace_offset)^N == 1 --
 *   the evaluation coset then meets the trace domain and a zerofier vanishes on it (the second is the exact condition
 *   when trace_offset != 1; the first is kept for every trace_offset).  A coefficient, boundary or periodic value >= p gives
 *   SMI_ERR_NON_CANONICAL; E < 4 gives SMI_ERR_EXPANSION_TOO_SMALL (Fri::new's assert, src/fri.rs:45: the quotients
 *   would not fit under the degree bound).
 *
 * Out of scope: binding a digest of the AIR (coefficients, boundary values, periodic values) into the transcript; keeping
 * the periodic tables on the device between calls; a multi-GPU twin.  (Row shifts above 1 are "AIR: transition windows"
 * below; zero-knowledge randomisers and the lift to extension challenges have sections of their own; degree-adjusted
 * terms are moot under out-of-domain sampling.)  The proofs of the entry
 * points of this section and the next draw every challenge from F_p: with a 30-bit modulus (the reference's choice) their
 * soundness is bounded by the field.  "Quartic extension" below has the field, the fold and the composition that lift the
 * challenges to 116 bits (smi_dev_air_prove_ext / smi_air_verify_ext), and lists what it leaves out.
 *
 * The entry points take the description as `const void *air` (a pointer to an smi_air): every parameter type of this
 * header is a scalar, a pointer to one, or one of the handle / configuration types the bindings already know. */
#define SMI_AIR_MAX_CONSTRAINTS 64
#define SMI_AIR_MAX_TERMS 1024
#define SMI_AIR_MAX_TERM_FACTORS 8
#define SMI_AIR_MAX_EXP 255
#define SMI_AIR_MAX_BOUNDARY_PER_COL 16
#define SMI_AIR_MAX_PERIODIC 16
#define SMI_AIR_MAX_WINDOW 4
typedef struct smi_air {
    uint32_t n_constraints, n_terms, n_factors, n_boundary;
    const uint32_t *constraint_first_term;  /* n_constraints + 1, ascending, [0] = 0, last = n_terms          */
    const uint64_t *term_coeff;             /* n_terms, canonical (< p)                                        */
    const uint32_t *term_first_factor;      /* n_terms + 1; a term with no factor is a constant                */
    const uint32_t *factor_var;             /* n_factors; < 2 * n_cols + 2 * n_periodic, the four kinds above  */
    const uint32_t *factor_exp;             /* n_factors; >= 1                                                 */
    const uint32_t *boundary_col;           /* n_boundary                                                      */
    const uint64_t *boundary_row;           /* n_boundary; < n, a (col, row) pair at most once                 */
    const uint64_t *boundary_value;         /* n_boundary; canonical                                           */
    uint32_t n_periodic;                    /* Q <= SMI_AIR_MAX_PERIODIC                                       */
    uint32_t window;                        /* S: 0 or 2 = two rows; 3 .. SMI_AIR_MAX_WINDOW: "AIR: transition windows" */
    const uint32_t *periodic_log_period;    /* n_periodic; l_j <= log_n                                        */
    const uint64_t *periodic_value;         /* the columns' values back to back, 2^l_j each, canonical         */
} smi_air;
/* Host only, no context (callable without a GPU, like smi_fri_num_rounds): validates air against cfg (log_n,
 * log_blowup, n_cols and the two offsets are read) for the modulus p and returns d and E.  Every AIR entry point
 * below runs it first. */
int smi_air_plan(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint32_t *degree, uint64_t *fri_expansion);
/* The text of the calling thread's last failed smi_air_plan ("" after a success). */
const char *smi_air_last_error(void);
/* The composition codeword on its own: d_lde = n_cols extended columns (stride elements apart, stride >= N), d_weights
 * = n_cols + n_constraints unreduced u64 challenges on the device, d_out = N elements.  The tables of the AIR are
 * copied to the device from pageable memory before the launch; nothing else synchronises.  The tiled kernel needs
 * d_lde 16-byte aligned, stride a multiple of 4 and a tile of all columns within 64 KB of LDS (n_cols * (64 + 2^log_blowup)
 * * 4 bytes at the least); otherwise a slower kernel without tiles computes the same codeword (one power per point). */
int smi_dev_air_compose(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_lde, size_t stride,
                        const uint64_t *d_weights, uint32_t *d_out);
/* The boundary points and every C_k on the n-1 row pairs of the trace itself (column-major, n apart; no extension, no
 * division).  *ok = 1, or 0 with the first violation in (kind, index, row) order -- boundary points (index = position
 * in the boundary lists) before transition constraints, lowest index, lowest row -- in *constraint and *row, and a
 * sentence naming it in smi_last_error.  *constraint is the boundary point's position or n_boundary + k.
 * Synchronises (the verdict comes back to the host). */
int smi_dev_air_check(smi_ctx *ctx, const void *air, uint32_t n_cols, uint32_t log_n, const uint32_t *d_trace_cols, int *ok,
                      uint32_t *constraint, uint64_t *row);
/* trace -> LDE -> one tree per column -> weights -> composition codeword -> Fri::prove at expansion factor E ->
 * openings.  cfg->row_leaves must be 0 (SMI_ERR_BAD_ARG; smi_dev_air_prove_rows below commits to one tree over the
 * rows); open_columns is taken as set.
 * Transcript: empty; for c < W absorb column root c, weight_c = challenge(); for k < K absorb k as 8 little-endian
 * bytes, weight_{W+k} = challenge(); FRI continues this transcript of 32W + 8K bytes (as smi_dev_fri_prove_fs would).
 * Proof bytes: the FRI objects, then per colinearity test s, with a = top[s] mod N/2 and b = a + N/2, the rows
 * FieldElements(col_0 .. col_{W-1}) at a, b and -- only when K > 0 -- at (a+B) mod N, (b+B) mod N; then for every s
 * and inside it every c the MerklePaths in the same position order.
 * stage_ms (optional) gets five values {lde, commit, compose, fri, open}.  Does not run smi_dev_air_check: a proof
 * made from a trace that violates the AIR is rejected by the verifier. */
int smi_dev_air_prove(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t *column_roots,
                      uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms);
/* Verifier of smi_dev_air_prove: Fri::verify of the leading objects with the transcript above and expansion factor E,
 * the length of the opening section, every authentication path against its column root, and the composition codeword
 * recomputed at x_a and x_b from the opened rows against the layer-0 triple.  *accept and smi_last_error as in
 * smi_stark_verify. */
int smi_air_verify(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t *column_roots, const uint8_t *proof,
                   size_t proof_len, int *accept);

/* ---- AIR over one row-committed tree ----------------------------------------------------------
 * The same statement, composition codeword, limits, status codes and smi_air_plan as above, with the extended trace
 * committed as ONE tree over its rows instead of W trees over its columns: a leaf costs ceil(W/4) + 8 mixes where the W
 * column leaves cost 9 W, there is one set of node levels instead of W, and a queried position is opened once instead of
 * W times.  The two calls below take cfg->row_leaves and cfg->open_columns as set, whatever they hold (smi_dev_air_prove
 * and smi_air_verify keep refusing row_leaves = 1).  n_cols <= 64 is also the widest row the leaf hash takes.
 *
 * Commitment.  One tree over N = n B leaves, leaf i = Hash::from_field_elements([lde[0][i] .. lde[W-1][i]]) (src/hash.rs:
 *   32-35 on the row's W u64s): the tree smi_dev_merkle_build_rows builds over the extended columns.  row_root (host,
 *   optional in the prover) is its root.
 * Transcript.  Empty; absorb the root (32 bytes); for j = 0 .. W+K-1 absorb j as 8 little-endian bytes, weight_j =
 *   challenge().  Column c has j = c, constraint k has j = W + k.  FRI continues this transcript of 32 + 8 (W + K) bytes
 *   (as smi_dev_fri_prove_fs would).  Periodic columns stay outside it.
 * Proof bytes.  The FRI objects at expansion factor E; then per colinearity test s, with a = top[s] mod N/2 and b = a +
 *   N/2, the rows FieldElements(col_0 .. col_{W-1}) at a, b and -- only when K > 0 -- at (a+B) mod N, (b+B) mod N (the
 *   column-tree proof's rows); then for every s ONE MerklePath per opened position, in the same position order, each
 *   log2 N digests deep.  With R = K ? 4 : 2 the opening section is t R (9 + 8 W) + t R (9 + 32 log2 N) bytes:
 *   t R (W - 1) (9 + 32 log2 N) fewer than the column-tree proof of the same statement.
 * stage_ms (optional) gets five values {lde, commit, compose, fri, open}, as in smi_dev_air_prove.
 * Verifier.  Transcript, weights and seed as above; Fri::verify at E; the exact length of the opening section, the tag
 *   and width of every record; every opened row hashed to its leaf from its 8-byte little-endian values as they stand in
 *   the proof; all t R paths against row_root; then the canonical check and the composition recomputed at x_a and x_b
 *   exactly as smi_air_verify does, periodic operands included (the same code).  *accept and smi_last_error as in
 *   smi_air_verify; a proof of the column-tree variant is rejected here and the other way round, since the transcripts
 *   differ even where the roots coincide (W = 1). */
int smi_dev_air_prove_rows(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t row_root[32],
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms);
int smi_air_verify_rows(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                        size_t proof_len, int *accept);

/* ---- Quartic extension: 116-bit challenges -----------------------------------------------------
 * The reference draws every challenge from F_p.  The standard remedy over a small NTT-friendly prime keeps the trace and
 * its commitment in the base field and takes the verifier's challenges -- the composition weights, the FRI folding
 * challenges -- from an extension; the composition codeword and FRI then live there.  This section has the field, FRI over
 * it and the AIR proof with weights from it; the entry points above are unchanged, byte for byte.
 *
 * The field.  F_q = F_p[X] / (X^4 - g) with p and g the context's; an element is four canonical residues c0 .. c3, low
 *   degree first: c0 + c1 X + c2 X^2 + c3 X^3.  X^4 - g is irreducible when p = 1 (mod 4) and g^((p-1)/2) = -1, which
 *   holds for both project primes with g = 3; q is 2^119.6 for 998244353 and 2^115.2 for 469762049.  Every entry point of
 *   this section refuses a p that is 3 (mod 4) or a g that is a square: SMI_ERR_BAD_ARG, the reason in smi_last_error
 *   (smi_ctx_create accepts neither today -- it wants 2^12 | p - 1 and a g of full 2-power order --, so through a context
 *   the check is a guard; smi_ext_mul and smi_ext_inv take any p and g and meet it).
 * Layout.  An extension codeword of L elements on the device is four coordinate columns of L u32 residues, `stride`
 *   elements apart: coordinate e of element i at d[e * stride + i].  That is the shape smi_dev_merkle_build_rows(n_cols = 4,
 *   col_stride = stride) hashes, so leaf i of its tree is Hash::from_field_elements([c0, c1, c2, c3]) of element i and costs
 *   the 9 mixes a base-field leaf costs.  The coordinates of a codeword are base-field codewords on the same domain:
 *   smi_dev_lde, smi_dev_ntt and a degree check apply coordinate by coordinate.  On the host an element is four
 *   consecutive u64.
 * Left out: the column-tree variant of the AIR proof; any smi_mgpu_* twin; out-of-domain sampling; zero-knowledge randomisers; binding an AIR digest into the transcript; the
 *   fold fused into the launch that hashes the row leaves (the base-field path's LEAF_FOLD) and a fused tail.  The query
 *   phase of the entry points of this section rests on t colinearity tests alone; "Grinding" below adds proof-of-work
 *   bits to it (smi_dev_fri_prove_ext_pow / smi_dev_air_prove_ext_pow).  A committed extension-field column (an auxiliary
 *   trace) exists in two forms, "Permutation argument" and "Lookup argument" below: one permutation per proof or one
 *   lookup per proof and not both, no periodic or next-row tuple members, no selectors, no column-tree or smi_mgpu_* twin. */
#define SMI_EXT_DEGREE 4
/* Host only, no context (like smi_air_plan): out = a * b and out = a^-1 in F_q, coordinates canonical.  SMI_ERR_BAD_ARG
 * for a (p, g) the section refuses (p not a prime < 2^31 that is 1 mod 4, g a square or outside 1 .. p-1),
 * SMI_ERR_NON_CANONICAL for a coordinate >= p, SMI_ERR_NO_INVERSE ("no inverse", src/ff.rs:171) for smi_ext_inv of zero.
 * out may alias an input. */
int smi_ext_mul(uint64_t p, uint64_t g, const uint64_t a[4], const uint64_t b[4], uint64_t out[4]);
int smi_ext_inv(uint64_t p, uint64_t g, const uint64_t a[4], uint64_t out[4]);
/* Fri::fold_codeword (src/fri.rs:57-91) over F_q.  d_in: an extension codeword of len elements (a power of two, 2 ..
 * 2^27) on offset * <omega>, coordinate columns stride >= len apart; d_alpha: the challenge's four coordinates as
 * unreduced u64 on the device, used mod p; d_out: len / 2 elements, columns out_stride >= len / 2 apart, not
 * overlapping d_in.  With lo = element i, hi = element i + len / 2 and x_i = offset * omega^i in F_p,
 *   out[i] = 2^-1 (lo + hi) + alpha * ((lo - hi) * 2^-1 * x_i^-1),
 * the product by alpha a full F_q product (16 multiplies and 4 reductions).  With alpha = (a, 0, 0, 0) every coordinate
 * is smi_dev_fri_fold of that coordinate.  16-byte accesses when d_in and d_out are 16-byte aligned and stride,
 * out_stride and len / 2 are multiples of 4; 4-byte accesses otherwise, same values.  Statuses as smi_dev_fri_fold. */
int smi_dev_fri_fold_ext(smi_ctx *ctx, const uint32_t *d_in, size_t len, size_t stride, const uint64_t *d_alpha, uint64_t offset,
                         uint64_t omega, uint32_t *d_out, size_t out_stride);
/* The composition codeword of "AIR" above under weights from F_q.  d_weights: 4 (n_cols + n_constraints) unreduced u64
 * on the device, coordinate e of weight j at 4 j + e (column c has j = c, constraint k has j = n_cols + k); d_out: four
 * coordinate columns of N elements, out_stride >= N apart.  term_c and tq_k are base-field values, so
 *   cw_e[i] = sum_c (w_{c,e} mod p) * term_c(x_i) + sum_k (w_{W+k,e} mod p) * tq_k(x_i)      for e = 0 .. 3:
 * coordinate e is what smi_dev_air_compose returns for the weight vector (w_{.,e}), bit for bit.  One launch evaluates
 * every quotient once per point and adds it into four accumulators, where four launches of smi_dev_air_compose read the
 * columns and walk the constraints four times.  Limits, statuses, periodic columns and the conditions of the tiled
 * kernel as for smi_dev_air_compose. */
int smi_dev_air_compose_ext(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_lde, size_t stride,
                            const uint64_t *d_weights, uint32_t *d_out, size_t out_stride);

/* Extension FRI.  Fri::commit / Fri::prove / Fri::verify (src/fri.rs:105-156, 250-311, 313-504) with codewords over
 * F_q.  The domain, the number of rounds (smi_fri_num_rounds), index sampling (src/fri.rs:168-213) and the authentication
 * paths are the reference's.  The differences:
 * Commitment.  Round r's tree is the row-leaf tree of its codeword (Layout above): one tree, 9 mixes a leaf.
 * Transcript.  The caller's prefix (any length, as in the *_fs calls); every round absorbs its root (32 bytes); on every
 *   round but the last, for e = 0 .. 3, the round then absorbs e as 8 little-endian bytes and takes challenge(): coordinate
 *   e of that round's alpha as an unreduced u64, used mod p.  The last round absorbs nothing after its root (the prover
 *   breaks before alpha, src/fri.rs:133-135).  The index seed is challenge() of the transcript as it then stands,
 *   through Hash::from_u64 as in src/fri.rs:272.  A round adds 64 bytes: the transcript's length mod 32 never changes.
 * Fold.  smi_dev_fri_fold_ext, the domain squared from round to round as in src/fri.rs:146-147.
 * Proof bytes (tags and widths of src/stream.rs:35-64).  R records of tag 0, the roots; one tag-2 record of 4 L_last
 *   values, the last codeword, element i at positions 4 i .. 4 i + 3; then per layer: per test one tag-2 record of 12
 *   values -- a, b, c, four coordinates each -- and after the layer's t records the three paths (a, b, c) per test.
 * Verifier.  The transcript above; the last record holds exactly 4 L_last values, L_last = N >> (R - 1); the row-leaf root
 *   of the last codeword equals the last root; EACH of its four coordinates, interpolated on the last domain, has degree
 *   <= L_last / E - 1; for every triple (x_a, a), (-x_a, b), (alpha, c) are colinear over F_q, that is
 *   (b - a)(alpha - x_a) = (c - a)(x_b - x_a) with x_a, x_b embedded from F_p; every path is checked against a leaf
 *   hashed from the element's four u64s as they stand in the proof.  A coordinate >= p anywhere is a rejection
 *   (*accept = 0 with a reason in smi_last_error), not a status.  A base-field proof is rejected here and an extension
 *   proof by smi_fri_verify_fs: the record widths differ.
 * smi_dev_fri_prove_ext: d_codeword = len = cfg->domain_length elements, coordinate columns stride >= len apart, len <=
 *   2^27; transcript = host bytes (NULL, 0: a fresh FiatShamir); *proof is malloc'ed (smi_free); top_indices (optional)
 *   gets the t top-level indices.  The round loop -- row tree, Fiat-Shamir round, fold -- the query and the emit are
 *   enqueued without a host round trip; the call synchronises once, for the copy-back.  Statuses as smi_dev_fri_prove_fs.
 * smi_fri_verify_ext: as smi_fri_verify_fs; pv_values gets FOUR values per entry of pv_indices (room for 8 t values). */
int smi_dev_fri_prove_ext(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_codeword,
                          size_t len, size_t stride, uint8_t **proof, size_t *proof_len, uint64_t *top_indices);
int smi_fri_verify_ext(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                       size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed);
/* AIR with extension weights, over one row-committed tree ("AIR over one row-committed tree" above: the same statement,
 * commitment, smi_air_plan, limits and status codes; cfg->row_leaves and cfg->open_columns are taken as set).
 * Transcript.  Empty; absorb the row root; for m = 0 .. 4 (W + K) - 1 absorb m as 8 little-endian bytes and take
 *   challenge().  Weight j is the element with coordinates challenge[4 j .. 4 j + 3] mod p; column c has j = c, constraint
 *   k has j = W + k.  Extension FRI continues this transcript of 32 + 32 (W + K) bytes.  Periodic columns stay outside it.
 * Composition.  smi_dev_air_compose_ext under those weights: four coordinate columns.
 * Proof bytes.  The extension-FRI objects at expansion factor E; then the opening section of smi_dev_air_prove_rows,
 *   unchanged: the same rows, the same single path per position, the same length formula.
 * Verifier.  As smi_air_verify_rows, with the four coordinates of the composition recomputed at x_a and x_b from the
 *   opened rows and the periodic operands and compared with the layer-0 triple's a and b.  A proof of
 *   smi_dev_air_prove_rows is rejected here and the other way round: the transcripts differ from the first weight on.
 * stage_ms as in smi_dev_air_prove_rows.  One host round trip remains, the one smi_dev_air_prove_rows has: the row root
 * comes back so that the weights and FRI's seed are computed on the host. */
int smi_dev_air_prove_ext(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t row_root[32],
                          uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms);
int smi_air_verify_ext(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                       size_t proof_len, int *accept);

/* ---- Grinding: proof-of-work bits for the query phase of the extension proofs ----------------
 * The extension lifts every challenge to 116 bits and more; the query phase still rests on t colinearity tests at
 * expansion factor E, about t log2(E) bits.  Grinding adds b bits to it: before the query indices are drawn the prover
 * finds a nonce whose hash with the transcript has b low zero bits and absorbs it; the verifier checks it with one hash.
 * The entry points above are unchanged, byte for byte; the ones below are the extension ones with a difficulty.
 *
 * Definition.  T = the transcript bytes (any length), b = the difficulty, 0 .. SMI_GRIND_MAX_BITS, nu = a u64 nonce.
 *   pow_ok(T, nu, b): with d = Hash::from_bytes(T || nu as 8 little-endian bytes) (src/hash.rs:7-30), the u64 read
 *     little-endian from d[24..32] has its b low bits zero.  b = 0 accepts every nonce.
 *   grind(T, b) = the SMALLEST nu with pow_ok(T, nu, b): proofs are deterministic, byte for byte.
 *   The check word is taken from bytes 24..31 because the index seed, challenge() of T || nu, is bytes 0..7 of the same
 *     digest: the seed's bits stay unconstrained.
 *   Search cap: 2^(b+6) tries unless the caller names one; beyond it the status is SMI_ERR_GRIND_EXHAUSTED (for a uniform
 *     hash the default cap is missed with probability e^-64).
 * Extension FRI with grinding.  The transcript of "Extension FRI" up to and including the last root; then nu =
 *   grind(transcript, b) is absorbed as 8 little-endian bytes; the index seed is challenge() of the transcript as it then
 *   stands, drawn and used exactly as before.  Proof bytes: the roots, the last-codeword record, then ONE record of tag 2
 *   with count 1 holding nu (17 bytes), then the layers as before.
 * Verifier.  After the last-codeword record the next record must be of tag 2 and hold exactly one value; nu is a u64, not
 *   a field element, so there is no canonical check; pow_ok must hold on the transcript after the last root, otherwise
 *   *accept = 0 with the reason "proof of work"; then the nonce is absorbed and the indices are sampled.  A proof ground
 *   at b verifies at every b' <= b (the b low zero bits include the b' low ones): the verifier's grind_bits is the least
 *   difficulty it demands.  A proof of the entry points without grinding is rejected here and the other way round.
 * AIR.  The transcript of smi_dev_air_prove_ext, the FRI above, the opening section unchanged: 17 bytes more than the
 *   proof of smi_dev_air_prove_ext.  stage_ms keeps five values; the search is part of `fri`.
 * grind_bits > SMI_GRIND_MAX_BITS is SMI_ERR_BAD_ARG (the reason in smi_last_error).
 * Left out: grinding on the base-field FRI / AIR entry points (their soundness is bounded by the 30-bit field anyway);
 *   smi_mgpu_* twins; grinding before the composition weights are drawn. */
#define SMI_GRIND_MAX_BITS 32
/* Host only, no context (like smi_air_plan): *ok = pow_ok(transcript, nonce, bits).  (NULL, 0) is the empty transcript. */
int smi_grind_check(const uint8_t *transcript, size_t transcript_len, uint64_t nonce, uint32_t bits, int *ok);
/* The search alone: *nonce = grind(transcript, bits).  The transcript is host memory; its state goes to the device, one
 * kernel searches, and the call synchronises once for the answer.  max_tries: the nonces 0 .. max_tries - 1 are tried, 0 =
 * the default cap 2^(bits+6); SMI_ERR_GRIND_EXHAUSTED when none of them is valid (the context stays usable). */
int smi_dev_grind(smi_ctx *ctx, const uint8_t *transcript, size_t transcript_len, uint32_t bits, uint64_t max_tries, uint64_t *nonce);
/* smi_dev_fri_prove_ext / smi_fri_verify_ext with grinding.  *nonce (optional) gets nu.  The search and the absorb run on
 * the device between the last codeword's emit and the index sampling: the prove gains no host round trip. */
int smi_dev_fri_prove_ext_pow(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_codeword,
                              size_t len, size_t stride, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, uint32_t grind_bits,
                              uint64_t *nonce);
int smi_fri_verify_ext_pow(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                           size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed,
                           uint32_t grind_bits);
/* smi_dev_air_prove_ext / smi_air_verify_ext with grinding. */
int smi_dev_air_prove_ext_pow(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t row_root[32],
                              uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits);
int smi_air_verify_ext_pow(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                           size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- Extension FRI, folding factor 4: one coset leaf per query and layer ------------------------
 * "Extension FRI" folds by 2: about 2 N leaves hashed over the rounds, and per query and layer three authentication paths.
 * Folding by 4 halves the round loop, hashes about N / 3 leaves of 16 values, and a query opens ONE path per layer: the
 * four points of a coset sit in one leaf, and the folded value needs no path of its own because it is an entry of the next
 * layer's opened coset.  The entry points above are unchanged, byte for byte; these are new ones beside them.
 * Field, codeword layout and transcript are those of "Extension FRI".  Grinding is always part of the stream: the nonce
 * record is always present, grind_bits is 0 .. SMI_GRIND_MAX_BITS, and at 0 the nonce is 0.
 *
 * Rounds.  R2 = smi_fri_num_rounds(cfg); R2 = 0 is refused as today (SMI_ERR_NO_ROUNDS).  F = (R2 - 1) / 2 (integer
 *   division) folds, F + 1 committed codewords.  Layer r has length n_r = N / 4^r, offset^(4^r) and omega^(4^r).  The last
 *   length L_last = n_F is at least the reference's last length and above E, so the degree bound L_last / E - 1 stays
 *   meaningful; the entropy statuses of smi_dev_fri_prove_ext apply to L_last.  A fold takes lengths 4 .. 2^27.  F = 0 is a
 *   proof without layers: one root, the codeword in the clear, the nonce.
 * Fold.  With q = n / 4, x = offset omega^i and iota = omega^q (a primitive fourth root of unity), output element i < q is
 *   P(alpha) for the unique P of degree < 4 over F_q with P(x iota^j) = cw[i + j q], j = 0 .. 3.  Equivalently -- the
 *   identity the tests check -- smi_dev_fri_fold_ext under alpha over (offset, omega, n), then under alpha^2 (the F_q square,
 *   reduced) over (offset^2, omega^2, n / 2), word for word: the outputs are canonical residues.
 * Commitment.  Layer r's tree has q_r = n_r / 4 leaves; leaf i is Hash::from_field_elements of 16 values: for e = 0 .. 3
 *   (outer) and j = 0 .. 3 (inner), coordinate e of element i + j q_r.  For a codeword whose columns are exactly n_r apart
 *   that is smi_dev_merkle_build_rows(n_cols = 16, col_stride = q_r, n = q_r): 12 mixes a leaf.  The last codeword is
 *   committed the same way.  A caller's first codeword with stride > len is compacted once (one copy of 16 N bytes).
 * Transcript.  Per codeword: absorb the root; on every one but the last draw four challenges exactly as "Extension FRI"
 *   does.  After the last root nu = grind(transcript, grind_bits) is absorbed; the index seed is challenge() of the
 *   transcript as it then stands, and the indices are sample_indices(seed, size = F ? N / 4 : N, reduced = L_last, t).
 * Indices.  i_0 = top mod q_0, i_{r+1} = i_r mod q_{r+1}.  The folded value of layer r's coset i_r is element i_r of
 *   codeword r + 1: slot j = i_r div q_{r+1} of layer r + 1's opened coset, and for r = F - 1 entry i_r of the last
 *   codeword.
 * Proof bytes.  F + 1 records of tag 0; one tag-2 record of 4 L_last values (element i at 4 i .. 4 i + 3); one tag-2
 *   record holding nu; then per layer r < F: t tag-2 records of 16 values in leaf order (the verifier hashes a record as
 *   it stands), then t paths of log2 q_r digests.  Length:
 *     33 (F + 1) + (9 + 32 L_last) + 17 + sum_{r < F} t (9 + 128) + t (9 + 32 log2 q_r)       (smi_fri_fold4_layout).
 * Verifier.  The checks that are "Extension FRI"'s keep its sentences: the roots, the last codeword's shape, canonical
 *   coordinates, its root (over coset leaves) and the degree of each coordinate, the proof of work; a coset record plays the
 *   triple's part ("Failed to extract triple values", "Expected triple of values", "triple: a coordinate is not
 *   canonical") and its path the part of path a.  Per layer: the t records, then -- from layer 1 on -- the previous layer's
 *   folds against this layer's slots, then the t paths; after the last layer its folds against the last codeword.  The one
 *   new sentence: "folded coset does not match the next layer".  A factor-2 proof is rejected here and a factor-4 proof by
 *   smi_fri_verify_ext_pow: the numbers of roots differ, or (R2 = 1) the leaves do.
 * AIR (row leaves, extension weights).  Transcript, weights, commitment and composition of smi_dev_air_prove_ext_pow; the
 *   FRI above.  Opening section, per test: a = top mod N / 4; the rows at a, a + N/4, a + N/2, a + 3N/4; when K > 0 the
 *   four rows at (. + B) mod N in the same order; then one path per opened position.  With R = K ? 8 : 4 the section is
 *   t R (9 + 8 W) + t R (9 + 32 log2 N) bytes.  The verifier recomputes the composition's four coordinates at all four
 *   points, periodic operands included, and compares them with the layer-0 coset record.  With F = 0 there is no such
 *   record: prover and verifier refuse the shape with SMI_ERR_BAD_ARG and a sentence in smi_last_error.
 * Left out: the permutation, lookup, args and xargs provers (they fold by 2); column trees; smi_mgpu_* twins; folding
 *   factors above 4; the fold fused into the launch that hashes the leaves. */
/* Host only, no context: the number of folds, the last codeword's length and the proof's length in bytes for cfg.
 * SMI_ERR_NO_ROUNDS when smi_fri_num_rounds is 0; the statuses of smi_fri_check for a malformed cfg. */
int smi_fri_fold4_layout(const smi_fri_cfg *cfg, uint64_t *folds, uint64_t *last_len, size_t *proof_len);
/* The fold above in one launch.  d_in: len elements (a power of two, 4 .. 2^27), columns stride >= len apart; d_out:
 * len / 4 elements, columns out_stride >= len / 4 apart, not overlapping d_in; d_alpha as for smi_dev_fri_fold_ext.  It
 * moves 80 bytes per output element where the two launches of smi_dev_fri_fold_ext move 144.  16-byte accesses when d_in
 * and d_out are 16-byte aligned and stride, out_stride and len / 4 are multiples of 4; 4-byte accesses otherwise, same
 * values.  omega must have order len for the Lagrange reading; the two-fold identity holds whenever omega^(len/2) = -1.
 * Statuses as smi_dev_fri_fold_ext. */
int smi_dev_fri_fold4_ext(smi_ctx *ctx, const uint32_t *d_in, size_t len, size_t stride, const uint64_t *d_alpha, uint64_t offset,
                          uint64_t omega, uint32_t *d_out, size_t out_stride);
/* smi_dev_fri_prove_ext_pow / smi_fri_verify_ext_pow at folding factor 4: the same parameters.  The round loop, the
 * search, the query and the emit are enqueued without a host round trip.  pv_indices needs room for 4 t entries and
 * pv_values for 16 t: the layer-0 cosets, element i_0 + j q_0 for j = 0 .. 3 per test. */
int smi_dev_fri_prove_ext_fold4(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_codeword,
                                size_t len, size_t stride, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, uint32_t grind_bits,
                                uint64_t *nonce);
int smi_fri_verify_ext_fold4(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                             size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed,
                             uint32_t grind_bits);
/* smi_dev_air_prove_ext_pow / smi_air_verify_ext_pow over the FRI above (AIR, above): the same parameters and stage_ms. */
int smi_dev_air_prove_ext_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t row_root[32],
                                uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits);
int smi_air_verify_ext_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                             size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- Permutation argument: a committed extension column ----------------------------------------
 * The AIR sections relate two consecutive rows.  This one relates rows far apart: it proves that two lists of row tuples
 * are equal as multisets -- "this column is a sorted copy of that one", memory consistency, copy constraints -- the way
 * every production STARK does: after the trace is committed the verifier draws challenges, the prover commits a second,
 * challenge-dependent column over F_q and the composition constrains it.  The entry points above are unchanged, byte for
 * byte.  Extension weights, extension FRI, row-committed trees and a nonce record always (grind_bits = 0 accepts nonce 0).
 *
 * Statement.  With m = width, l_j = left_col[j], r_j = right_col[j] and T the trace (n = 2^log_n rows): as multisets over
 *   all n rows, { (T[l_0][r], .., T[l_{m-1}][r]) } = { (T[r_0][r], .., T[r_{m-1}][r]) }.  One permutation per proof.
 * The column.  With alpha, gamma in F_q:  f_L(r) = gamma + sum_j alpha^j T[l_j][r], f_R likewise with r_j;
 *   rho[r] = f_L(r) / f_R(r);  z[0] = 1, z[r+1] = z[r] rho[r] for r = 0 .. n-2.  The multisets are equal iff (up to about
 *   n m / q) the product closes: z[n-1] rho[n-1] = 1.  z is four coordinate columns of n residues ("Layout" above).
 * Auxiliary constraints.  The column's own transition WRAPS AROUND: z(w x) f_R(x) - z(x) f_L(x) vanishes on all n rows and
 *   is divided by x^n - tau^n (the main AIR's transitions keep their no-wrap rule); the boundary quotient is
 *   (z(x) - 1) / (x - tau).  Both have degree 2: d = max(d_air, 2), D and E follow as in smi_air_plan.
 * Protocol.
 *   1. smi_dev_lde of the trace, the tree over its rows: root_1.
 *   2. The transcript starts empty and absorbs root_1.
 *   3. For m = 0 .. 7 absorb m as 8 little-endian bytes and take challenge() -> c[m];  alpha = (c0 .. c3) mod p, gamma =
 *      (c4 .. c7) mod p.
 *   4. z on the device from the unextended trace (smi_dev_perm_column).
 *   5. smi_dev_lde of its four coordinate columns, smi_dev_merkle_build_rows(n_cols = 4) over them: root_2.
 *   6. Absorb root_2.
 *   7. For m = 0 .. 4 (W + K + 2) - 1 absorb 8 + m as 8 little-endian bytes and take challenge().  Weight j has the
 *      coordinates 4 j .. 4 j + 3; column c has j = c, constraint k has j = W + k, the auxiliary boundary quotient j = W + K,
 *      the auxiliary transition quotient j = W + K + 1.  The transcript is then 32 + 64 + 32 + 32 (W + K + 2) bytes.
 *   8. The codeword is smi_dev_air_compose_ext under the weights 0 .. W + K - 1, plus
 *        w_{W+K} (z(x_i) - 1) / (x_i - tau)  +  w_{W+K+1} (z(w x_i) f_R(x_i) - z(x_i) f_L(x_i)) / (x_i^n - tau^n),
 *      f_L(x_i) = gamma + sum_j alpha^j lde[l_j][i], z(w x_i) = the extended column at index (i + B) mod N, every product
 *      in F_q.
 *   9. Extension FRI with grinding at E, continuing that transcript ("Grinding" above).
 *  10. Openings: two sections, each in the layout of smi_dev_air_prove_rows with R = 4 positions per test (a, b, (a + B) mod
 *      N, (b + B) mod N; always 4, whatever K): tree 1 with rows of W values, then tree 2 with rows of 4 values.
 *   Proof bytes: the extension-FRI objects with their nonce record, then t 4 (9 + 8 W) + t 4 (9 + 32 log2 N) bytes, then
 *   t 4 (9 + 32) + t 4 (9 + 32 log2 N) bytes.  Two host round trips remain, one per root: each root comes back so that the
 *   challenges that depend on it are computed on the host.
 * Verifier (host).  In this order: the same transcript; smi_fri_verify_ext_pow's checks at E; the exact lengths of both
 *   sections, every record's tag and width; the leaves hashed from the bytes as they stand; all paths against root_1 and
 *   root_2; every opened value canonical, the z coordinates included (a violation is a rejection with a reason, not a
 *   status); the composition recomputed at x_a and x_b from the opened rows -- the main part by the code smi_air_verify_ext
 *   runs, the two auxiliary quotients in host F_q arithmetic -- against the layer-0 triple.  A proof of
 *   smi_dev_air_prove_ext_pow is rejected here and the other way round, and so is a proof checked under another
 *   smi_air_perm: the challenges are the same, the recomputed composition is not.
 * The prover does not refuse a trace whose product does not close (*closes = 0); the verifier rejects that proof, as with
 *   smi_dev_air_check and a violated AIR.
 * Limits (SMI_ERR_BAD_ARG, the reason in smi_air_last_error / smi_last_error): width in 1 .. SMI_PERM_MAX_WIDTH; every
 *   column index < n_cols; log_n >= 1; everything smi_air_plan refuses.
 * Left out: more than one permutation per proof; next-row tuple members in this single form (selectors and periodic
 *   members: "Argument list with selectors and periodic members" below; a member read one row later: "Argument list:
 *   next-row operands"); a permutation together with a
 *   lookup ("Lookup argument" below); a column-tree or smi_mgpu_* twin; the auxiliary quotients fused into the main composition launch (a follow-up: they run
 *   as a second streaming kernel over the four coordinate columns).  Several arguments, and permutations together with
 *   lookups, are what "Argument list" below adds; these entry points stay at one. */
#define SMI_PERM_MAX_WIDTH 8
typedef struct smi_air_perm {
    uint32_t width, reserved0;      /* m, 1 .. SMI_PERM_MAX_WIDTH; explicit padding, ignored */
    const uint32_t *left_col;       /* m column indices < n_cols                              */
    const uint32_t *right_col;      /* m column indices < n_cols; may overlap left_col        */
} smi_air_perm;
/* Host only (like smi_air_plan, which it runs first): validates perm against cfg and returns d = max(d_air, 2) and E.
 * `perm` is a pointer to an smi_air_perm, passed as the AIR is. */
int smi_air_plan_perm(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *perm, uint32_t *degree, uint64_t *fri_expansion);
/* The column z of the trace d_trace_cols (n_cols columns of n = 2^log_n residues, n apart) under challenges[0 .. 7] (host,
 * unreduced): d_z gets four coordinate columns of n residues, z_stride >= n apart.  Each lane takes four consecutive rows
 * and inverts its four denominators with one F_q inversion; the prefix product is a multi-launch scan (workgroup products,
 * one workgroup scanning them, propagation) with no wait of one workgroup on another.  16-byte accesses when d_trace_cols
 * and d_z are 16-byte aligned, n >= 4 and z_stride is a multiple of 4; 4-byte accesses otherwise, same values.
 * *closes (optional) = 1 iff z[n-1] rho[n-1] = 1.  If some f_R(r) is zero the status is SMI_ERR_NO_INVERSE, smi_last_error
 * names the smallest such r, and the context stays usable.  Synchronises (both verdicts come back to the host). */
int smi_dev_perm_column(smi_ctx *ctx, const void *perm, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, const uint64_t *challenges,
                        uint32_t *d_z, size_t z_stride, int *closes);
/* The codeword of step 8: smi_dev_air_compose_ext under the first 4 (W + K) of d_weights (4 (W + K + 2) unreduced u64 on the
 * device), then one streaming launch that adds the two auxiliary quotients into the four coordinate columns.  d_z_lde: the
 * extended column z, four coordinate columns of N residues z_stride >= N apart; challenges as for smi_dev_perm_column.
 * The streaming launch makes 16-byte accesses, four points per lane, when d_lde, d_z_lde and d_out are 16-byte aligned and
 * the three strides are multiples of 4; 4-byte accesses otherwise, same values. */
int smi_dev_air_compose_perm(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *perm, const uint32_t *d_lde, size_t stride,
                             const uint32_t *d_z_lde, size_t z_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                             size_t out_stride);
/* The prover of the protocol above.  roots (host, optional) gets root_1 then root_2; stage_ms (optional) gets six values
 * {lde, commit, perm, compose, fri, open} -- perm is the column, its extension and its tree; *closes (optional) as above.
 * cfg->row_leaves and cfg->open_columns are taken as set.  A zero denominator is SMI_ERR_NO_INVERSE as above. */
int smi_dev_air_prove_perm(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *perm, const uint32_t *d_trace_cols, uint8_t *roots,
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, int *closes);
int smi_air_verify_perm(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *perm, const uint8_t *roots, const uint8_t *proof,
                        size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- Lookup argument: LogUp over a committed extension column ----------------------------------
 * The permutation argument states that two lists of row tuples are equal as multisets.  This one states that every tuple of
 * one list OCCURS in the other -- range checks, opcode and instruction tables, byte decompositions, S-box tables, memory-
 * address membership -- by the logarithmic-derivative argument (LogUp): sum_r 1 / (X + l_r) = sum_t M_t / (X + t_t) as
 * rational functions iff every l_r is some t_t and M counts them.  The construction follows "Permutation argument" step
 * by step with a running SUM s in place of the running product z; the entry points above are unchanged, byte for byte.
 *
 * Statement.  With m = width in 1 .. SMI_LOOKUP_MAX_WIDTH, l_j = lookup_col[j], t_j = table_col[j], mult_col a trace column
 *   that is none of those 2 m, and T the trace (n = 2^log_n rows): for every row r the tuple (T[l_0][r], .., T[l_{m-1}][r])
 *   occurs among the n table tuples (T[t_0][t], .., T[t_{m-1}][t]).  Column mult_col holds the multiplicities: M[t] = the
 *   number of rows r whose lookup tuple equals table tuple t; when several table rows hold the same tuple it is credited
 *   to the lowest such t and the others hold 0.  M[t] <= n <= 2^27 < p: the characteristic does not interfere.  A short table
 *   is padded by repeating an entry; lookups that are not wanted are padded by repeating a table entry.  One lookup per
 *   proof, and not together with a permutation.
 * The column.  With alpha, gamma in F_q:  f_L(r) = gamma + sum_j alpha^j T[l_j][r], f_T likewise with t_j;
 *   s[0] = 0, s[r+1] = s[r] + 1 / f_L(r) - M[r] / f_T(r).  The statement holds iff (up to about n m / q) the sum closes:
 *   s[n-1] + 1 / f_L(n-1) - M[n-1] / f_T(n-1) = 0.  s is four coordinate columns of n residues.
 * Auxiliary constraints.  The boundary quotient is s(x) / (x - tau); the transition WRAPS AROUND:
 *   ((s(w x) - s(x)) f_L(x) f_T(x) - f_T(x) + M(x) f_L(x)) / (x^n - tau^n).  The transition has degree 3: d = max(d_air, 3),
 *   D >= 2, E = B / D, so log_blowup >= 3 is needed for E >= 4 (SMI_ERR_EXPANSION_TOO_SMALL otherwise).
 * Protocol.  The ten steps of the permutation argument with s in place of z:
 *   1. smi_dev_lde of the trace -- mult_col included, so the multiplicities are committed before alpha and gamma are
 *      drawn --, the tree over its rows: root_1.
 *   2-3. The transcript absorbs root_1; eight challenges under the counters 0 .. 7: alpha = (c0 .. c3) mod p, gamma =
 *      (c4 .. c7) mod p.
 *   4-6. s on the device from the unextended trace (smi_dev_lookup_column), smi_dev_lde of its four coordinate columns, the
 *      tree over their rows: root_2, absorbed.
 *   7. 4 (W + K + 2) weight challenges under the counters 8 + i; weight W + K is the auxiliary boundary quotient's, W + K + 1
 *      the auxiliary transition quotient's.  The transcript is 32 + 64 + 32 + 32 (W + K + 2) bytes, as for a permutation.
 *   8. The codeword is smi_dev_air_compose_ext under the weights 0 .. W + K - 1 plus
 *        w_{W+K} s(x_i) / (x_i - tau)
 *        + w_{W+K+1} ((s(w x_i) - s(x_i)) f_L(x_i) f_T(x_i) - f_T(x_i) + M(x_i) f_L(x_i)) / (x_i^n - tau^n),
 *      f_L(x_i) = gamma + sum_j alpha^j lde[l_j][i], M(x_i) = lde[mult_col][i], s(w x_i) = the extended column at index
 *      (i + B) mod N, every product in F_q.
 *   9. Extension FRI with grinding at E, continuing that transcript.
 *  10. Openings: two sections with R = 4, tree 1 with rows of W values, tree 2 with rows of 4 values.  Proof bytes and
 *      lengths as for a permutation proof.
 * Verifier (host).  The order of checks of smi_air_verify_perm, its sentences starting "lookup openings:".  A permutation
 *   proof checked here is rejected on the composition, and the other way round: transcript and layout are the same, the
 *   recomputed composition is not.  So is a proof checked under another smi_air_lookup.
 * The prover takes the trace as const with mult_col filled (smi_dev_lookup_multiplicities fills it for a caller who has
 *   not).  It does not refuse a wrong M or a missing lookup: *closes = 0 and the verifier rejects that proof.
 * Limits (SMI_ERR_BAD_ARG, the reason in smi_air_last_error / smi_last_error): width in 1 .. SMI_LOOKUP_MAX_WIDTH; every
 *   column index < n_cols; mult_col none of the tuple columns; log_n >= 1; everything smi_air_plan refuses.
 * Left out: several lookups, or several looked-up tuples sharing one table; next-row tuple members in this single form
 *   (selectors and periodic members: "Argument list with selectors and periodic members" below; a member read one row later:
 *   "Argument list: next-row operands"); a lookup together with a permutation; the auxiliary quotients fused into the main composition launch; a
 *   column-tree or smi_mgpu_* twin.  Several lookups, each with a multiplicity column of its own, and lookups together
 *   with permutations are what "Argument list" below adds, several looked-up tuples sharing one table and one multiplicity
 *   column what "Shared-table lookups" adds; these entry points stay at one. */
#define SMI_LOOKUP_MAX_WIDTH 8
typedef struct smi_air_lookup {
    uint32_t width, mult_col;       /* m, 1 .. SMI_LOOKUP_MAX_WIDTH; the multiplicity column, < n_cols */
    const uint32_t *lookup_col;     /* m column indices < n_cols                                        */
    const uint32_t *table_col;      /* m column indices < n_cols; may overlap lookup_col                */
} smi_air_lookup;
/* Host only (like smi_air_plan, which it runs first): validates lookup against cfg and returns d = max(d_air, 3) and E.
 * `lookup` is a pointer to an smi_air_lookup, passed as the AIR is. */
int smi_air_plan_lookup(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *lookup, uint32_t *degree, uint64_t *fri_expansion);
/* A helper for callers, never called by the prover: d_mult (n residues, zeroed by the call) gets the multiplicities M of the
 * statement above for the trace d_trace_cols (n_cols columns of n = 2^log_n residues, n apart; column mult_col is not
 * read).  Two launches over an open-addressing table of 2 n row indices: the table tuples are inserted with the lowest row
 * winning, then every lookup tuple is probed for and counted with an atomic add.  Every probe loop is bounded by the
 * table's size and no lane waits on another.  The result does not depend on the hash function or on scheduling.  If some
 * lookup tuple is in no table row the status is SMI_ERR_LOOKUP_MISSING, smi_last_error names the smallest such row, d_mult
 * holds the counts of the others, and the context stays usable.  Synchronises. */
int smi_dev_lookup_multiplicities(smi_ctx *ctx, const void *lookup, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, uint32_t *d_mult);
/* The column s of the trace under challenges[0 .. 7] (host, unreduced): d_s gets four coordinate columns of n residues,
 * s_stride >= n apart.  The three launches of smi_dev_perm_column -- workgroup sums, one workgroup scanning them,
 * propagation; no wait of one workgroup on another -- with an additive scan; each lane takes four consecutive rows and
 * inverts its four products f_L f_T with one F_q inversion.  16-byte accesses when d_trace_cols and d_s are 16-byte aligned,
 * n >= 4 and s_stride is a multiple of 4; 4-byte accesses otherwise, same values.  *closes (optional) = 1 iff the sum
 * closes.  If some f_L(r) or f_T(r) is zero the status is SMI_ERR_NO_INVERSE, smi_last_error names the smallest such r and
 * which of the two it was, and the context stays usable.  Synchronises. */
int smi_dev_lookup_column(smi_ctx *ctx, const void *lookup, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, const uint64_t *challenges,
                          uint32_t *d_s, size_t s_stride, int *closes);
/* The codeword of step 8; arguments and access rules as for smi_dev_air_compose_perm, d_s_lde the extended column s. */
int smi_dev_air_compose_lookup(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *lookup, const uint32_t *d_lde, size_t stride,
                               const uint32_t *d_s_lde, size_t s_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                               size_t out_stride);
/* The prover of the protocol above.  roots (host, optional) gets root_1 then root_2; stage_ms (optional) gets six values
 * {lde, commit, lookup, compose, fri, open} -- lookup is the column, its extension and its tree; *closes (optional) as
 * above.  cfg->row_leaves and cfg->open_columns are taken as set.  A zero denominator is SMI_ERR_NO_INVERSE as above. */
int smi_dev_air_prove_lookup(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *lookup, const uint32_t *d_trace_cols, uint8_t *roots,
                             uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, int *closes);
int smi_air_verify_lookup(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *lookup, const uint8_t *roots, const uint8_t *proof,
                          size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- Argument list: several permutation and lookup arguments in one proof ----------------------
 * The two sections above put ONE challenge-dependent F_q column in the second row tree.  A real statement needs several --
 * a memory-consistency permutation, an opcode-table lookup and a range check or two over the same trace -- and separate
 * proofs would repeat the trace's extension, its tree and FRI, and would not bind the arguments to one committed trace.
 * This variant takes a list of A arguments, 1 <= A <= SMI_ARGS_MAX, each a permutation or a lookup, in any mix and any
 * order.  The entry points above are unchanged, byte for byte.
 *
 * Statement.  Argument a is the statement of "Permutation argument" (kind SMI_ARG_PERM: a_col = left_col, b_col =
 *   right_col) or of "Lookup argument" (kind SMI_ARG_LOOKUP: a_col = lookup_col, b_col = table_col, and its own mult_col) as
 *   written there, with its own column lists.  Several lookups that share one multiplicity column are left out.
 * Challenges.  All arguments share one alpha and one gamma.  No further separation is needed: every argument owns a column
 *   that closes on its own, and each column's two quotients enter the composition under weights of their own.
 * The columns.  Argument a has the F_q column c_a -- z for a permutation, s for a lookup --, with its section's recurrence
 *   unchanged.  The A columns are stored as 4 A coordinate columns; argument a occupies the columns 4 a .. 4 a + 3.
 * Degree.  d = max(d_air, 2 if any argument is a permutation, 3 if any is a lookup); D and E follow as in smi_air_plan, so a
 *   list with a lookup needs log_blowup >= 3.
 * Protocol.  The ten steps of the permutation argument with these differences:
 *   4-6. All A columns on the device from the unextended trace (smi_dev_args_columns), ONE smi_dev_lde over the 4 A
 *      coordinate columns, ONE tree over their rows (n_cols = 4 A): root_2, absorbed.
 *   7. 4 (W + K + 2 A) weight challenges under the counters 8 + i; weight W + K + 2 a is the boundary quotient of argument
 *      a, weight W + K + 2 a + 1 its wrapping transition quotient.  The transcript is 32 + 64 + 32 + 32 (W + K + 2 A) bytes.
 *   8. The codeword is smi_dev_air_compose_ext under the weights 0 .. W + K - 1 plus the 2 A auxiliary quotients, each
 *      exactly as its own section defines it.
 *  10. Openings: two sections with R = 4, tree 1 with rows of W values, tree 2 with rows of 4 A values: the second section is
 *      t 4 (9 + 32 A) + t 4 (9 + 32 log2 N) bytes.
 *   With A = 1 every byte coincides with the proof of smi_dev_air_prove_perm or smi_dev_air_prove_lookup.
 * Verifier (host).  The order of checks of smi_air_verify_perm, its sentences starting "argument openings:".  A proof
 *   checked under the list in another order, under a changed argument or under fewer arguments is rejected.
 * The prover does not refuse a column that does not close: bit a of *closes is set iff argument a closes, and the verifier
 *   rejects a proof with a column that does not.
 * Limits (SMI_ERR_BAD_ARG, the reason in smi_air_last_error / smi_last_error): count in 1 .. SMI_ARGS_MAX; kind 0 or 1;
 *   every argument by its own section's limits, the reason naming the argument's index; everything smi_air_plan refuses.
 * Left out: next-row tuple members in this list without selectors (selectors and periodic members are what "Argument
 *   list with selectors and periodic members" below adds, members read one row later what "Argument list: next-row
 *   operands" adds to that section's entry points, several tuples under one multiplicity column what "Shared-table lookups" adds to that section's
 *   entry points; these entry points stay as they are and refuse a kind with a tuple count); the auxiliary
 *   quotients fused into the main composition launch; a column-tree or smi_mgpu_* twin; a wave-level scan. */
#define SMI_ARGS_MAX 8
#define SMI_ARG_PERM 0
#define SMI_ARG_LOOKUP 1
typedef struct smi_air_arg {
    uint32_t kind;            /* SMI_ARG_PERM = 0, SMI_ARG_LOOKUP = 1 */
    uint32_t width;           /* m, 1 .. 8                             */
    uint32_t mult_col;        /* ignored for a permutation             */
    uint32_t reserved0;       /* explicit padding, ignored             */
    const uint32_t *a_col;    /* left / lookup columns                 */
    const uint32_t *b_col;    /* right / table columns                 */
} smi_air_arg;
typedef struct smi_air_args {
    uint32_t count;           /* A, 1 .. SMI_ARGS_MAX                  */
    uint32_t reserved0;
    const smi_air_arg *arg;
} smi_air_args;
/* Host only (like smi_air_plan, which it runs first): validates the list against cfg and returns d and E.  `args` is a
 * pointer to an smi_air_args, passed as the AIR is. */
int smi_air_plan_args(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *args, uint32_t *degree, uint64_t *fri_expansion);
/* The A columns of the trace under challenges[0 .. 7] (host, unreduced): d_c gets 4 A coordinate columns of n residues,
 * c_stride >= n apart.  Exactly three launches whatever A is: the block launch with the argument as the second grid
 * dimension, the scan launch with one workgroup per argument, the propagation; no wait of one workgroup on another.
 * 16-byte accesses when d_trace_cols and d_c are 16-byte aligned, n >= 4 and c_stride is a multiple of 4; 4-byte accesses
 * otherwise, same values.  *closes (optional): bit a is set iff argument a closes.  A zero denominator is
 * SMI_ERR_NO_INVERSE; smi_last_error names the smallest key 16 row + 2 a + side (side 0: f_L, side 1: f_R or f_T) by its
 * row, argument and side, and the context stays usable.  Synchronises.  smi_dev_lookup_multiplicities stays the helper for
 * the multiplicities: a caller runs it once per lookup argument. */
int smi_dev_args_columns(smi_ctx *ctx, const void *args, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, const uint64_t *challenges,
                         uint32_t *d_c, size_t c_stride, uint32_t *closes);
/* The codeword of step 8: smi_dev_air_compose_ext under the first 4 (W + K) of d_weights (4 (W + K + 2 A) unreduced u64 on
 * the device), then ONE streaming launch that adds the 2 A auxiliary quotients with one 16-byte read-modify-write per
 * codeword coordinate.  d_c_lde: the 4 A extended coordinate columns, c_stride >= N apart.  Access rules as for
 * smi_dev_air_compose_perm. */
int smi_dev_air_compose_args(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *args, const uint32_t *d_lde, size_t stride,
                             const uint32_t *d_c_lde, size_t c_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                             size_t out_stride);
/* The prover of the protocol above.  roots (host, optional) gets root_1 then root_2; stage_ms (optional) gets six values
 * {lde, commit, args, compose, fri, open} -- args is the columns, their extension and their tree; *closes (optional) is the
 * mask above.  cfg->row_leaves and cfg->open_columns are taken as set.  Two host round trips, as for one argument. */
int smi_dev_air_prove_args(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *args, const uint32_t *d_trace_cols, uint8_t *roots,
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, uint32_t *closes);
int smi_air_verify_args(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *args, const uint8_t *roots, const uint8_t *proof,
                        size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- Argument list with selectors and periodic members ------------------------------------------
 * The arguments of the three sections above fire on every row and read committed trace columns only.  A real trace looks an
 * operand up only on the rows where an opcode flag is set, looks it up in a PUBLIC table (a range 0 .. 255, an opcode
 * table) and relates "the selected rows of these columns" to "the selected rows of those".  This variant of "Argument list"
 * gives every argument two optional selectors and lets tuple members and selectors be periodic columns of the AIR.  The
 * entry points above are unchanged, byte for byte, and keep launching the kernels they launch.
 *
 * Operands.  An operand is a variable in the AIR's own numbering (W = n_cols, Q = n_periodic): var = c with c < W is trace
 *   column c at this row, var = 2 W + j with j < Q periodic column j at this row.  The two next-row kinds (W <= var < 2 W,
 *   var >= 2 W + Q) are refused; a this-row variable read one row later is SMI_ARG_NEXT_ROW | var ("Argument list: next-row
 *   operands" below).  On the trace the value V(r) is T[c][r] or v_j[r mod P_j]; on the evaluation coset V(x_i)
 *   is lde[c][i] or pi_j(x_i), the extended periodic table read modulo its length P_j B exactly as the main composition
 *   reads it ("AIR" above).
 * Argument a.  kind, width m in 1 .. 8, the operand lists a_var[m] and b_var[m], the selectors a_sel and b_sel -- an operand
 *   each, or SMI_ARG_NO_SELECTOR for the constant 1 -- and for a lookup mult_col, a trace column that is none of the
 *   argument's trace operands and none of its selectors.  S_a, S_b are the selector values, M = T[mult_col];
 *   f_L = gamma + sum_j alpha^j V_{a_var[j]}, f_R / f_T likewise with b_var.  All arguments share alpha and gamma.
 * Permutation.  g_L = 1 + S_a (f_L - 1), g_R = 1 + S_b (f_R - 1);  z[0] = 1, z[r+1] = z[r] g_L(r) / g_R(r); the argument
 *   closes iff z[n-1] g_L(n-1) / g_R(n-1) = 1.  Boundary quotient (z(x) - 1) / (x - tau); wrapping transition quotient
 *   (z(w x) g_R(x) - z(x) g_L(x)) / (x^n - tau^n).  Degree contributed: 2 with no selector, 3 with one or two.
 * Lookup.  s[0] = 0, s[r+1] = s[r] + S_a(r) / f_L(r) - M(r) S_b(r) / f_T(r); the argument closes iff the next step returns
 *   to 0.  Boundary quotient s(x) / (x - tau); wrapping transition quotient
 *   ((s(w x) - s(x)) f_L f_T - S_a f_T + M S_b f_L) / (x^n - tau^n), of degree 3 with or without selectors.
 * What is proved.  The two identities above, rational or multiplicative.  With selectors that hold only 0 and 1 that is the
 *   multiset statement (permutation) or the inclusion statement (lookup) over the SELECTED rows of either side.  Forcing a
 *   trace selector to be 0 / 1 is the AIR's business (a transition or boundary constraint s^2 - s = 0 of the caller's); a
 *   periodic selector is public, part of the statement, and needs no constraint.
 * Degree.  d = max(d_air, the arguments' contributions); D and E follow as in smi_air_plan_args.
 * Zero denominators.  A zero f_L or f_T of a lookup is SMI_ERR_NO_INVERSE on every row, selected or not; so is a zero g_R
 *   of a permutation.  The key stays 16 row + 2 a + side, the smallest key is reported, the context stays usable.
 * Transcript, second tree, weights, FRI, grinding, openings, proof layout, byte counts: exactly those of "Argument list".
 *   Periodic columns stay outside the transcript, as everywhere.
 * Verifier (host).  The order of checks of smi_air_verify_args and its sentences.  The 2 A auxiliary quotients are recomputed
 *   at x_a and x_b from the opened rows in host F_q arithmetic; the periodic operands at those points come from the code
 *   smi_air_verify_ext uses.  A proof checked under a list that differs in one selector, or in one member being periodic
 *   instead of a trace column, is rejected on the composition.
 * Anchor.  A list in which no argument has a selector or a periodic operand yields every byte of smi_dev_air_prove_args for
 *   the same list; the roots, the columns and the codeword are equal too.
 * Limits (SMI_ERR_BAD_ARG, the reason names the argument): those of "Argument list"; every operand a this-row variable,
 *   bare or under SMI_ARG_NEXT_ROW;
 *   mult_col < n_cols, none of the argument's trace operands, none of its selectors; everything smi_air_plan refuses.
 * Left out: a column-tree or smi_mgpu_* twin.  (Members and selectors read one row later: "Argument list: next-row
 *   operands" below, through these entry points.  Several looked-up tuples under one table, one
 *   multiplicity column and one running sum: "Shared-table lookups" below, through these entry points.)
 *   (FRI at the full blowup and a lookup list at log_blowup = 2 are what "Out-of-domain sampling with an argument list"
 *   below adds.) */
#define SMI_ARG_NO_SELECTOR 0xffffffffu
#define SMI_ARG_NEXT_ROW 0x40000000u    /* operand = SMI_ARG_NEXT_ROW | v, v a this-row variable: v one row later ("Argument list: next-row operands") */
#define SMI_ARG_MAX_TUPLES   4
#define SMI_ARG_TUPLES_SHIFT 8      /* kind = SMI_ARG_LOOKUP | (J - 1) << SMI_ARG_TUPLES_SHIFT, J in 1 .. SMI_ARG_MAX_TUPLES ("Shared-table lookups") */
typedef struct smi_air_xarg {
    uint32_t kind;            /* SMI_ARG_PERM = 0, SMI_ARG_LOOKUP = 1; bits 8 .. 15: J - 1 */
    uint32_t width;           /* m, 1 .. 8                                          */
    uint32_t mult_col;        /* a trace column; ignored for a permutation          */
    uint32_t reserved0;       /* explicit padding, ignored                          */
    const uint32_t *a_var;    /* left / lookup operands, m variables of this row    */
    const uint32_t *b_var;    /* right / table operands                             */
    uint32_t a_sel, b_sel;    /* an operand, or SMI_ARG_NO_SELECTOR                 */
} smi_air_xarg;
typedef struct smi_air_xargs {
    uint32_t count;           /* A, 1 .. SMI_ARGS_MAX                               */
    uint32_t reserved0;
    const smi_air_xarg *arg;
} smi_air_xargs;
/* Host only (like smi_air_plan, which it runs first): validates the list against cfg and air and returns d and E.  `xargs`
 * is a pointer to an smi_air_xargs, passed as the AIR is. */
int smi_air_plan_xargs(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint32_t *degree, uint64_t *fri_expansion);
/* smi_dev_lookup_multiplicities for argument a of the list, which must be a lookup: d_mult (n residues, zeroed by the call)
 * gets M.  Only table rows with S_b != 0 are inserted, only lookup rows with S_a != 0 are counted, M at an unselected table
 * row is 0; SMI_ERR_LOOKUP_MISSING names the smallest SELECTED row whose tuple is in no selected table row.  Of air the
 * periodic columns are read (periods <= n).  Two launches, every probe loop bounded by the table's size.  Synchronises. */
int smi_dev_xargs_multiplicities(smi_ctx *ctx, const void *air, const void *xargs, uint32_t a, const uint32_t *d_trace_cols, uint32_t n_cols,
                                 uint32_t log_n, uint32_t *d_mult);
/* smi_dev_args_columns under the recurrences above: three launches whatever A is -- a block launch of its own with the
 * argument as the second grid dimension, then the scan and propagation launches of smi_dev_args_columns.  The raw periodic
 * values go to the device first.  Access rules, *closes, the zero-denominator report as there. */
int smi_dev_xargs_columns(smi_ctx *ctx, const void *air, const void *xargs, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n,
                          const uint64_t *challenges, uint32_t *d_c, size_t c_stride, uint32_t *closes);
/* smi_dev_air_compose_args with the quotients above: smi_dev_air_compose_ext, then ONE streaming launch that reads the
 * periodic operands from the tables the main composition of the same call has built. */
int smi_dev_air_compose_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint32_t *d_lde, size_t stride,
                              const uint32_t *d_c_lde, size_t c_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                              size_t out_stride);
/* The prover: smi_dev_air_prove_args step by step (two host round trips, stage_ms {lde, commit, args, compose, fri, open}). */
int smi_dev_air_prove_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint32_t *d_trace_cols, uint8_t *roots,
                            uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, uint32_t *closes);
int smi_air_verify_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint8_t *roots, const uint8_t *proof,
                         size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- Shared-table lookups: several tuples, one multiplicity, one running sum --------------------
 * In the sections above every looked-up tuple is an argument of its own: a multiplicity column in the trace, four committed
 * coordinate columns, two auxiliary quotients (three under zero knowledge) and one of the SMI_ARGS_MAX slots.  A range check of
 * four byte columns against one table 0 .. 255 takes half the list.  LogUp needs one multiplicity column and one running sum
 * for all of them, and this section gives that to the smi_*_xargs entry points of every variant -- row leaves, DEEP, coset
 * leaves, zero knowledge -- without a new entry point or struct.  smi_air_arg (the list without selectors) keeps refusing.
 *
 * Statement.  A shared lookup has J looked-up tuples of width m, one table tuple, one multiplicity column and one running
 *   sum.  Tuple j has the operands a_j[0 .. m) and an optional selector S_j; the table side is b_var, b_sel, mult_col as in
 *   "Argument list with selectors and periodic members".  With f_j = gamma + sum_i alpha^i V(a_j[i]) and f_T as there,
 *       s[0] = 0,   s[r+1] = s[r] + sum_{j<J} S_j(r) / f_j(r)  -  M(r) S_b(r) / f_T(r);
 *   it closes iff the step after the last row returns to 0 (under zero knowledge: iff c_a[n_a] = 0).  M[t] counts the
 *   (row, tuple) pairs that hit table row t; two tuples of one row may hit the same table row.  The boundary quotient and
 *   the closing quotient of the zero-knowledge variant are a lookup's.  With P = prod_j f_j and
 *   Nn = sum_j S_j prod_{i != j} f_i the wrapping transition quotient is
 *       ((s(w x) - s(x)) P f_T  -  Nn f_T  +  (M S_b) P) / (x^n - tau^n);
 *   with J = 1 that is the lookup of that section, word for word.
 * Encoding.  smi_air_xarg.kind = SMI_ARG_LOOKUP | (J - 1) << SMI_ARG_TUPLES_SHIFT: the low byte is the kind, bits 8 .. 15 hold
 *   J - 1, bits 16 and above are 0.  J = 1 is the value SMI_ARG_LOOKUP itself: every list written before means what it meant.
 *   For J >= 2: a_var holds the J m operands, tuple-major, followed by J selector entries (an operand each, or
 *   SMI_ARG_NO_SELECTOR); a_sel is SMI_ARG_NO_SELECTOR; width is m; mult_col is none of the operands and none of the
 *   selectors.  reserved0 stays ignored.
 * Degree.  A shared lookup contributes J + 2 to d in smi_air_plan_xargs and smi_air_plan_deep_xargs and J + 3 in
 *   smi_air_plan_deep_zk_xargs (3 and 4 for J = 1, as before); D, E, D' and every layout follow as they do there.  So the
 *   saving in columns is conditional on the blowup at hand:
 *     row leaves, fold 2   E = B / D >= 4 is needed: J = 2, 3 (D = 4) run from log_blowup 4, J = 4 (D = 8) from log_blowup 5,
 *                          where a single lookup runs from 3;
 *     DEEP, no zk          J = 2, 3 give D = 4, J = 4 gives D = 8, where a list of single lookups has D = 2: the composition
 *                          gains segments while the trace and the second tree lose columns;
 *     DEEP with zk         J = 2 keeps D = 4, exactly as a single lookup does -- sharing is free there; J = 3, 4 give D = 8;
 *     an AIR whose own degree reaches J + 2 (J + 3 under zk) pays nothing anywhere.
 * Kernels.  The tuples are folded one at a time into the pair (Nn, P) <- (Nn f_j + S_j P, P f_j) from (0, 1), so that a row
 *   has ONE denominator P f_T and one numerator Nn f_T - (M S_b) P: the column build keeps its one F_q inversion per lane
 *   of four rows, and registers grow by two F_q values a row, not by J.  A list in which some argument has J >= 2 takes
 *   sibling launches (xargs_block_shared_kernel, air_xargs_compose_shared_kernel, air_zk_xargs_compose_shared_kernel,
 *   xargs_count_shared_kernel) that get the tuples in a structure of their own; every other list launches the kernels it
 *   launched, unchanged.  The scan, propagation, insert and tail launches are shared.
 * Multiplicities.  smi_dev_xargs_multiplicities / _rows: the insert launch is unchanged; in the count launch a lane probes
 *   once per selected tuple of its row.  SMI_ERR_LOOKUP_MISSING names the smallest row and, within it, the smallest tuple.
 * Zero denominators.  A zero f_j or f_T is SMI_ERR_NO_INVERSE on every row, selected or not; the smallest (row, argument,
 *   side) is reported, side = j for f_j and J for f_T, and for J >= 2 the sentence names the tuple.  A list without a
 *   shared lookup keeps its key 16 row + 2 a + side and its sentence.
 * Verifiers.  The order of checks and the sentences of each variant, unchanged; the transition numerator above is
 *   recomputed from the opened rows (row leaves) or at z (DEEP, coset leaves, zero knowledge).  A proof checked under
 *   J - 1 tuples, one changed operand, one dropped selector or the J single lookups is rejected.
 * Limits (SMI_ERR_BAD_ARG, the reason names the argument): tuple bits on a permutation; J > SMI_ARG_MAX_TUPLES; a set a_sel
 *   for J >= 2; one of the AIR's own next-row variables in any tuple or selector; J n >= p, where the multiplicities could wrap (reachable for
 *   J >= 2 alone, and only through the entry points that take log_n without a blowup: a plan keeps n <= (p - 1) / 4);
 *   kind = 2, or bits above the second byte, with the sentence of "Argument list".
 * Measured (profiles/shared_lookup_time.log, profiles/shared_lookup_kernel_resources.log): DESIGN.md section 11.
 * Left out: next-row operands under zero knowledge; several tables in one argument; sharing across arguments (a joint closing condition
 *   over several columns); more than 4 tuples; smi_mgpu_* twins; the list without selectors (smi_air_args); an AIR digest
 *   in the transcript. */

/* ---- Argument list: next-row operands -----------------------------------------------------------
 * The lists above relate cells of ONE row.  What LogUp is most often asked for relates a row to its successor: (state[r],
 * input[r], state[r+1]) is a row of a public transition table -- a DFA, an opcode decoder, a carry table -- or a sorted column
 * is compared with its own shift.  Until here that took a copy column d[r] = c[r+1] and a transition constraint binding it: a
 * column extended, hashed, opened at every query and at z and z w only because an operand could not say "next".  Every proof
 * variant that takes a list already carries what such an operand needs -- the row-leaf provers open the rows a + B and b + B,
 * the DEEP provers open every trace column at z w, every verifier evaluates pi_j(w x) -- so no proof layout, record count,
 * transcript shape or degree changes.
 *
 * Statement.  An operand may be a this-row variable read one row later, cyclically: on the trace V(r) = T[c][(r + 1) mod n] or
 *   v_j[(r + 1) mod P_j]; as a polynomial f_c(w x) or pi_j(w x); on the evaluation coset lde[c][(i + B) mod N], or the extended
 *   periodic table read at (i + B) mod L_j.  The wrap is deliberate -- the arguments' own transition quotients wrap too; a
 *   caller who does not want row n - 1 to see row 0 deselects it with a (periodic) selector.  Allowed in every operand
 *   position: the members of either side, the J tuples of a shared lookup, a_sel, b_sel, the per-tuple selectors.  Not as
 *   mult_col, which stays a plain trace column.
 * Encoding.  operand = SMI_ARG_NEXT_ROW | v with v a this-row variable (c < W, or 2 W + j).  The AIR's own next-row variable
 *   numbers stay refused with their sentence, flagged or not; SMI_ARG_NO_SELECTOR keeps its meaning; any other high bit leaves
 *   v outside the AIR's variables and is refused as that.  mult_col is compared with the operands after the flag is stripped:
 *   next(mult_col) as a member or a selector is refused with the sentences of mult_col.
 * Degree.  Unchanged: d, D, E and every layout function return what they return for the same list with the flags removed.
 * Kernels.  A NEXT template parameter on xargs_block_kernel, air_xargs_compose_kernel, xargs_insert_kernel /
 *   xargs_count_kernel and their shared siblings; a list without a next-row operand launches the instantiations it always
 *   launched (profiles/next_row_members_kernel_resources.log: their registers, LDS and scratch are the parent's, the new ones
 *   have no scratch).  Column build: a lane owns four rows and needs the rows one further; three are in its own 16-byte load,
 *   the fourth is one 4-byte load of the next word, row 0 for the last lane of the column.  Composition: the operand is read
 *   at (i + B) mod N, where the launch reads the auxiliary columns' next row already; one aligned 16-byte load, as before.
 *   Multiplicities: both launches hash and compare the cell at (row + 1) mod n; SMI_ERR_LOOKUP_MISSING and the
 *   zero-denominator key name the row that READS, with their numbering.
 * Who takes such a list.  smi_air_plan_xargs, smi_air_plan_deep_xargs and the three layouts; smi_dev_xargs_multiplicities,
 *   smi_dev_xargs_columns, smi_dev_air_compose_xargs; smi_dev_air_prove_xargs / smi_air_verify_xargs (the operand at x_a from
 *   the opened row a + B, and pi_j(w x_a)); smi_dev_air_prove_deep_xargs / smi_air_verify_deep_xargs and the _fold4 pair (the
 *   operand at z from the record's v_c = f_c(z w), and pi_j(z w)).  Proof bytes, record counts and the order and text of every
 *   rejection are unchanged; a proof checked under the list with one flag removed or moved is rejected on the composition
 *   (row leaves) or the consistency check (DEEP).
 * Who refuses (SMI_ERR_BAD_ARG, "<argument>: <operand> is a next-row operand", before any device work):
 *   smi_air_plan_deep_zk_xargs and everything behind it (the layout, smi_dev_air_compose_zk_xargs, the prover, the verifier);
 *   smi_dev_xargs_multiplicities_rows.  smi_air_args (no selectors) keeps refusing every operand that is no column; windows
 *   above 2 keep being refused with lists.
 * Measured (profiles/next_row_members_time.log; n = 2^20, B = 8, t = 32, coset leaves): the 9-column list of the README plus one
 *   lookup with a next-row member proves in 6.618 ms and 260011 bytes, the same statement with a copy column and its constraint
 *   in 6.822 ms and 261099 bytes.  The NEXT column build takes 0.107 ms where the plain one takes 0.097 (the extra 4-byte load,
 *   131 VGPRs for 128), the NEXT composition 0.657 for 0.652.  DESIGN.md section 11.
 * Left out: next-row operands under zero knowledge; shifts above one row in lists; the single permutation() / lookup() forms
 *   and smi_air_args; smi_mgpu_* twins; opening at z w only the columns some operand or constraint reads there. */

/* ---- Out-of-domain sampling (DEEP): FRI at the full blowup -------------------------------------
 * The AIR proofs above recompute the composition at the t queried positions only, so their FRI runs at E = B / D, an AIR
 * with E < 4 is refused, and every test opens the next rows (a + B, b + B) as well.  Here the constraint check moves to one
 * random point z of F_q ("out-of-domain sampling", listed as left out by "AIR" and "Quartic extension" above: this section
 * is that step).  The composition is committed in D segments of degree < n, everything FRI sees has degree < n, FRI runs at
 * E = B whatever the AIR's degree is, the + B rows disappear and every AIR with D <= B is provable -- mimc at
 * log_blowup = 2, for one.  The variant stands next to smi_dev_air_prove_ext_pow: row leaves, extension weights, extension
 * FRI folding by 2, the nonce record always present (grind_bits = 0 accepts nonce 0).  It takes a plain AIR -- boundary
 * points, transition constraints, periodic columns -- and has no permutation, lookup or argument-list form and no
 * folding factor 4.  Every entry point above is unchanged, byte for byte.
 *
 * Notation of "AIR": W, K, Q, n, B, N = n B, tau, h, w = omega_n, x_i = h omega_N^i, f_c the trace polynomials, term_c,
 *   tq_k, pi_j; d and D as smi_air_plan computes them.
 * Plan (smi_air_plan_deep).  smi_air_plan's checks, except its bound on E, which plays no part.  Refused: D > B
 *   (SMI_ERR_BAD_ARG: the composition has degree < D n and must fit the N points); B < 4 (SMI_ERR_EXPANSION_TOO_SMALL);
 *   4 D > 64 (SMI_ERR_BAD_ARG: the widest row the leaf hash takes).
 * Prover.
 *   1. smi_dev_lde of the trace, the row tree over it: root_1.  The transcript starts empty and absorbs root_1.
 *   2. For m = 0 .. 4 (W + K) - 1 absorb m as 8 little-endian bytes and take challenge(): the composition weights of
 *      smi_dev_air_prove_ext.  H = the codeword of smi_dev_air_compose_ext under them, four coordinate columns.
 *   3. Segments.  The coefficients of every coordinate of H on the coset h <omega_N> (an inverse coset transform of size N);
 *      H(x) = sum_{j<D} x^(j n) H_j(x) with H_j the coefficients j n .. (j + 1) n - 1 (those at and above D n are dropped: an
 *      honest H has none); every coordinate of every H_j extended back to the N points, 4 D columns; the second tree is
 *      smi_dev_merkle_build_rows(n_cols = 4 D) over them, row value 4 j + e = coordinate e of H_j.  Its root is root_2,
 *      which is absorbed.
 *   4. For m = 4 (W + K) .. 4 (W + K) + 3 absorb m and take challenge(): the coordinates of z mod p.  If coordinates 1 .. 3
 *      are all zero z lies in F_p: the prover returns SMI_ERR_BAD_ARG with a sentence and the verifier rejects with the same
 *      sentence (probability about p^-3).  For every other z each denominator below is non-zero, since the n-th roots of
 *      unity of F_q all lie in F_p.
 *   5. u_c = f_c(z) and v_c = f_c(z w) for c < W from the trace polynomials' coefficients (smi_dev_ntt, inverse, offset tau),
 *      s_j = H_j(z) for j < D.  One tag-2 record of 4 (2 W + D) values u_0 .. u_{W-1}, v_0 .. v_{W-1}, s_0 .. s_{D-1}, four
 *      canonical coordinates each (the v_c are sent when K = 0 as well).  Its payload, 32 (2 W + D) bytes without tag and
 *      count, is absorbed.
 *   6. For m = 4 (W + K) + 4 .. 4 (W + K) + 4 + 4 (2 W + D) - 1 absorb m and take challenge(): gamma_c, gamma'_c, gamma''_j in
 *      record order, four coordinates each, used mod p.  The transcript is then 32 (3 + W + K + 2 (2 W + D)) bytes.
 *   7. The DEEP codeword over F_q, i < N:
 *        Q(x_i) = sum_c gamma_c (f_c(x_i) - u_c) / (x_i - z) + sum_c gamma'_c (f_c(x_i) - v_c) / (x_i - z w)
 *               + sum_j gamma''_j (H_j(x_i) - s_j) / (x_i - z),   of degree < n.
 *   8. Extension FRI with grinding continues that transcript on h <omega_N> at expansion factor B.
 *   9. Openings.  Per test a = top mod N/2 and b = a + N/2; two sections in the layout of smi_dev_air_prove_rows with R = 2:
 *      tree 1 with rows of W values, then tree 2 with rows of 4 D values.  No + B rows.
 * Proof bytes.  The out-of-domain record, the FRI objects with their nonce record, the two sections:
 *   9 + 32 (2W + D) + len_FRI(N, B, t) + 2t (9 + 8W) + 2t (9 + 32 log2 N) + 2t (9 + 32D) + 2t (9 + 32 log2 N)
 *   (smi_air_deep_layout).  The two roots go to the caller, 64 bytes, as in the permutation variant.
 * Host round trips of the prover: three -- root_1, root_2, and the out-of-domain values.
 * Verifier (smi_air_verify_deep), all arithmetic in F_q, in this order, each rejection with a sentence of its own in
 *   smi_last_error: the out-of-domain record has the exact count and canonical coordinates; the same transcript (z in F_p is
 *   rejected); out-of-domain consistency,
 *        sum_c w_c term_c(z) + sum_k w_{W+k} tq_k(z) = sum_j z^(j n) s_j,
 *   with term_c(z) = (u_c - I_c(z)) / Z_c(z) (u_c without boundary points), tq_k(z) = C_k(u, v, pi(z), pi(z w))
 *   (z - tau w^(n-1)) / (z^n - tau^n) and pi_j(z) = q_j((z / tau)^(n / P_j)), the constraints evaluated over F_q operands on
 *   the host; Fri::verify over F_q at E = B with the proof of work; the lengths, tags and widths of both sections; every path
 *   against its root, leaves hashed from the bytes as they stand; canonical values in the opened rows; Q(x_a) and Q(x_b)
 *   recomputed from the opened rows against the layer-0 triple's a and b.  A proof of smi_dev_air_prove_ext_pow is rejected
 *   here, and a proof of this variant by smi_air_verify_ext_pow.
 * Soundness accounting and measured times: DESIGN.md section 11, "Out-of-domain sampling".
 * Left out: folding factor 4 (it comes with coset leaves, below); column trees; smi_mgpu_* twins; zero-knowledge randomisers; binding an AIR digest into the
 *   transcript; the segment extension fused into the leaf hash.  (Permutation, lookup and argument lists are what
 *   "Out-of-domain sampling with an argument list" below adds; these entry points stay as they are.) */
/* Host only (like smi_air_plan): the plan above -> d and D. */
int smi_air_plan_deep(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint32_t *degree, uint32_t *segments);
/* Host only: the plan, and the length in bytes of the proof of that shape (num_colinearity_tests is read as well). */
int smi_air_deep_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, size_t *proof_len);
/* n_cols columns of n_coeffs base-field coefficients (low degree first, `stride` elements apart, any n_coeffs >= 1) at
 * n_points = 1 or 2 points of F_q (points: four canonical coordinates each, host): out[4 (c n_points + k) + e] = coordinate
 * e of column c at point k (host).  Both points come from one pass over the coefficients.  Two launches whatever n_cols is:
 * workgroups reduce chunks of 1024 coefficients against a table of the points' powers (four base-field multiplies per
 * coefficient and point), a second small launch combines the partial sums; no atomics.  16-byte loads when d_coeffs is
 * 16-byte aligned and stride a multiple of 4, 4-byte loads otherwise.  Synchronises (the values come back to the host). */
int smi_dev_poly_eval_ext(smi_ctx *ctx, const uint32_t *d_coeffs, uint32_t n_cols, size_t n_coeffs, size_t stride, const uint64_t *points,
                          uint32_t n_points, uint64_t *out);
/* The DEEP codeword of step 7 on its own.  cfg: n_cols = W, log_n, log_blowup (>= 2) and lde_offset are read.  d_lde: W
 * extended columns `stride` apart; d_seg: 4 n_segments segment columns seg_stride apart (column 4 j + e = coordinate e of
 * H_j); z: four canonical coordinates, not all of 1 .. 3 zero; ood: the record's 4 (2 W + D) canonical values; challenges:
 * as many unreduced u64 (gamma, gamma', gamma''), all three on the host; d_out: four coordinate columns out_stride apart.
 * One streaming launch, 4 (W + 4 D) + 16 bytes a point; the F_q inversions are batched eight to a lane.  16-byte accesses
 * when the three bases are 16-byte aligned and the three strides multiples of 4, 4-byte accesses with the same values
 * otherwise.  The table of the gammas is copied to the device from pageable memory before the launch. */
int smi_dev_deep_compose(smi_ctx *ctx, const smi_stark_cfg *cfg, uint32_t n_segments, const uint32_t *d_lde, size_t stride, const uint32_t *d_seg,
                         size_t seg_stride, const uint64_t z[4], const uint64_t *ood, const uint64_t *challenges, uint32_t *d_out, size_t out_stride);
/* smi_dev_poly_eval_ext at the n_shifts = 1 .. SMI_AIR_MAX_WINDOW points z, z w, .. z w^(n_shifts - 1) ("AIR: transition
 * windows"): z four canonical coordinates, w a canonical base-field element, out[4 (c n_shifts + s) + e] = coordinate e of
 * column c at z w^s.  One pass over the coefficients serves all shifts: the first launch holds a table of powers per point
 * (16 n_shifts words a lane), four base-field multiplies per coefficient and shift; the second combines the partial sums;
 * no atomics; the same 16-byte / 4-byte load rule.  For n_shifts <= 2 the values are those of smi_dev_poly_eval_ext at z, z w.
 * smi_dev_poly_eval_ext itself keeps its limit of two arbitrary points. */
int smi_dev_poly_eval_ext_shifts(smi_ctx *ctx, const uint32_t *d_coeffs, uint32_t n_cols, size_t n_coeffs, size_t stride, const uint64_t z[4], uint64_t w,
                                 uint32_t n_shifts, uint64_t *out);
/* smi_dev_deep_compose under a window of S = window rows, 2 .. SMI_AIR_MAX_WINDOW ("AIR: transition windows"):
 *   Q(x_i) = sum_{s<S} sum_c gamma_{s,c} (f_c(x_i) - u_{s,c}) / (x_i - z w^s) + sum_j gamma''_j (H_j(x_i) - s_j) / (x_i - z).
 * ood: the record's 4 (S W + D) canonical values, u_{s,c} s-major, then s_j; challenges: as many unreduced u64 in that
 * order.  One streaming launch; the 4 S denominators of a lane share one F_q inversion; the access rule of
 * smi_dev_deep_compose.  With window = 2 every output word is smi_dev_deep_compose's (the same kernel over the same table). */
int smi_dev_deep_compose_window(smi_ctx *ctx, const smi_stark_cfg *cfg, uint32_t window, uint32_t n_segments, const uint32_t *d_lde, size_t stride,
                                const uint32_t *d_seg, size_t seg_stride, const uint64_t z[4], const uint64_t *ood, const uint64_t *challenges, uint32_t *d_out,
                                size_t out_stride);
/* The prover above.  roots (optional): root_1 then root_2, 64 bytes; ood (optional): the record's 4 (2 W + D) values --
 * 4 (S W + D) for an AIR with a window of S rows ("AIR: transition windows"), which is what the buffer must hold;
 * stage_ms (optional) gets seven values {lde, commit, compose, segments, ood, fri, open} -- "ood" holds the evaluations,
 * their round trip and the DEEP codeword. */
int smi_dev_air_prove_deep(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t *roots, uint64_t *ood,
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits);
int smi_air_verify_deep(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t *roots, const uint8_t *proof, size_t proof_len, int *accept,
                        uint32_t grind_bits);

/* ---- AIR: transition windows of up to four rows -------------------------------------------------
 * A transition constraint of "AIR" reads a column at this row and the next.  With smi_air.window = S in {3, 4} it reads the
 * rows r .. r + S - 1, so a[r+2] = a[r+1] + a[r] is one column and no copy column is committed, hashed and opened.  window 0
 * and 2 both mean the two-row statement above, byte for byte; 1 and anything above SMI_AIR_MAX_WINDOW are SMI_ERR_BAD_ARG
 * with a sentence that names the window.
 * Variables (W = n_cols, Q = n_periodic): var = s W + c is trace column c at row r + s, var = S W + s Q + j periodic column
 *   j at row r + s, s < S; for S = 2 that is the numbering of "AIR".  factor_var < S (W + Q).
 * Where constraints hold: on the windows that start at rows 0 .. n - S, no wrap; n >= S is required.
 *   tq_k(x) = C_k(...) * prod_{s=1..S-1} (x - tau w^(n-s)) / (x^n - tau^n);   boundary quotients do not change.
 *   On the evaluation coset the operand of shift s is lde[c][(i + s B) mod N], and pi_j(w^s x_i) = table_j[(i + s B) mod L_j].
 * Degree and segments: the quotient's degree is at most d (n - 1) + (S - 1) - n.  d is reported as before; D starts from the
 *   smallest power of two >= max(1, d - 1) and is doubled while D n <= d (n - 1) + (S - 1) - n.  For S = 2 it never doubles;
 *   it doubles once for (d, S) in {(2, 3), (2, 4), (3, 4)} (1 -> 2, 1 -> 2, 2 -> 4) and for no other pair.  E = B / D and the
 *   DEEP refusals (D > B, 4 D > 64) follow from that D.
 * Who takes such an AIR: smi_air_plan, smi_dev_air_compose, smi_dev_air_compose_ext, smi_dev_air_check (windows r .. r + S - 1
 *   for r <= n - S, periodic operands v_j[(r + s) mod P_j], the same first-violation order), smi_air_plan_deep, the two DEEP
 *   layouts, smi_dev_air_prove_deep / smi_air_verify_deep and smi_dev_air_prove_deep_fold4 / smi_air_verify_deep_fold4.
 *   Every other prover, verifier and plan -- column trees, rows, ext, pow, fold4 without DEEP; perm, lookup, args, xargs and
 *   their DEEP forms; both zero-knowledge variants -- returns SMI_ERR_BAD_ARG with a sentence naming the window, before any
 *   device work.
 * DEEP proofs under a window.  A window row is one more out-of-domain point: the queried rows do not change.
 *   Record: u_{s,c} = f_c(z w^s), s-major (s = 0 .. S - 1, then c < W), then s_j: 4 (S W + D) values, 32 (S W + D) payload
 *     bytes; for S = 2 that is u then v.  Step 6 draws 4 (S W + D) challenges in record order, the counter continuing.
 *   Q(x_i) = sum_{s<S} sum_c gamma_{s,c} (f_c(x_i) - u_{s,c}) / (x_i - z w^s) + sum_j gamma''_j (H_j(x_i) - s_j) / (x_i - z).
 *   Proof and transcript lengths: those of the two DEEP sections with 2 W replaced by S W in the record and in the challenge
 *     count, and nothing else: 9 + 32 (S W + D) + ..., transcript 32 (3 + W + K + 2 (S W + D)).  Openings, FRI, grinding,
 *     roots, host round trips and the stage_ms order are unchanged.
 *   Verifiers: the record's count 4 (S W + D); C_k over the S opened rows and pi_j(z w^s); the exemption product at z;
 *     Q(x_a), Q(x_b) with S denominators; the order of checks and the sentences of their sections.  A proof checked under
 *     another window is rejected at the record count when S W differs, and at the consistency check otherwise.
 * Kernels: the tiled composition stages a halo of (S - 1) B points (the direct kernel takes over where no tile fits);
 *   smi_dev_poly_eval_ext_shifts and smi_dev_deep_compose_window are declared with "Out-of-domain sampling" above.
 * Measured (profiles/air_window_kernel_resources.log, profiles/air_window_time.log): DESIGN.md section 11.
 * Left out: windows above four rows; opening only the (column, shift) pairs that a constraint reads; argument lists and
 *   zero knowledge over wider windows (the zk row counts k_t depend on the number of opened functionals); the non-DEEP
 *   provers; smi_mgpu_* twins.  (A list reads one row further through its operands: "Argument list: next-row operands".) */

/* ---- Out-of-domain sampling with an argument list ----------------------------------------------
 * The argument-list provers recompute the composition at the queried positions, so a list with a lookup (degree 3) needs
 * log_blowup >= 3, runs FRI at E = B / 2 and opens four rows of two trees a test; "Out-of-domain sampling" above runs FRI at
 * E = B and opens two rows a test, but takes a plain AIR.  This variant is out-of-domain sampling for an smi_air_xargs list
 * (the superset form: a list without selectors is written as one with SMI_ARG_NO_SELECTOR everywhere): the A auxiliary F_q
 * columns are opened at z and z w next to the trace, as production provers of this shape open main and auxiliary trace.
 * A lookup list is provable at log_blowup = 2.  Every entry point above is unchanged, byte for byte, and keeps launching
 * the kernels it launches.
 *
 * Notation of "Out-of-domain sampling" and "Argument list": W, K, A, D, n, B, N = n B, tau, h, w = omega_n, x_i = h omega_N^i,
 *   c_a the polynomial of argument a's column, NW = W + K + 2 A weights.
 * Plan (smi_air_plan_deep_xargs).  smi_air_plan_xargs's checks without its bound on E; d by that section's rule (a
 *   permutation with a selector counts 3, any lookup 3); D the next power of two >= d - 1; refused as smi_air_plan_deep
 *   refuses, with its sentences: D > B, B < 4, 4 D > 64.  4 A <= 32 always fits a leaf row.
 * Prover.
 *   1. smi_dev_lde of the trace, the row tree over it: root_1, absorbed by an empty transcript.
 *   2. Counters 0 .. 7: alpha and gamma, as in step 3 of "Permutation argument".
 *   3. The A columns (the launches of smi_dev_xargs_columns), ONE smi_dev_lde over their 4 A coordinate columns, ONE row tree
 *      over those (n_cols = 4 A): root_2, absorbed.
 *   4. Counters 8 + m, m < 4 NW: the composition weights of "Argument list" step 7.  H = the codeword of
 *      smi_dev_air_compose_xargs on the N points; the columns' next-row values come from index (i + B) mod N.
 *   5. The segments of H exactly as in step 3 of "Out-of-domain sampling"; the third tree is over their 4 D columns: root_3,
 *      absorbed.
 *   6. Counters 8 + 4 NW + e, e < 4: the coordinates of z.  A z in F_p is refused by prover and verifier with the sentence of
 *      "Out-of-domain sampling".
 *   7. One tag-2 record of 4 (2 W + 2 A + D) values, four canonical coordinates each, in this order: u_c = f_c(z) and
 *      v_c = f_c(z w) for c < W; a_a = c_a(z) and b_a = c_a(z w) for a < A; s_j = H_j(z) for j < D.  c_a(z) is assembled on
 *      the host as sum_e X^e coord_{a,e}(z) from the coefficients of the unextended coordinate columns (an inverse transform
 *      of size n at offset tau), the way s_j is.  The payload is absorbed.
 *   8. The following 4 (2 W + 2 A + D) counters: gamma_c, gamma'_c, delta_a, delta'_a, gamma''_j in record order.  The
 *      transcript is then 32 (6 + NW + 2 (2 W + 2 A + D)) bytes.
 *   9. The DEEP codeword over F_q, i < N:
 *        Q(x_i) = sum_c gamma_c (f_c(x_i) - u_c) / (x_i - z) + sum_c gamma'_c (f_c(x_i) - v_c) / (x_i - z w)
 *               + sum_a delta_a (c_a(x_i) - a_a) / (x_i - z) + sum_a delta'_a (c_a(x_i) - b_a) / (x_i - z w)
 *               + sum_j gamma''_j (H_j(x_i) - s_j) / (x_i - z),   of degree < n.
 *  10. Extension FRI with grinding continues that transcript at E = B, folding by 2.
 *  11. Openings.  Per test a = top mod N/2 and b = a + N/2; three sections in the R = 2 row layout: rows of W values (tree 1),
 *      rows of 4 A values (tree 2), rows of 4 D values (tree 3).  No + B rows.
 * Proof bytes (smi_air_deep_xargs_layout):
 *   9 + 32 (2W + 2A + D) + len_FRI(N, B, t) + 2t (9 + 8W) + 2t (9 + 32 log2 N) + 2t (9 + 32A) + 2t (9 + 32 log2 N)
 *     + 2t (9 + 32D) + 2t (9 + 32 log2 N).
 *   The three roots go to the caller, 96 bytes.  Host round trips of the prover: four -- the three roots and the record.
 * Verifier (smi_air_verify_deep_xargs, host).  The checks of smi_air_verify_deep in their order, over three sections (their
 *   sentences start "deep argument openings:"), with the consistency check extended to
 *        sum_c w_c term_c(z) + sum_k w_{W+k} tq_k(z) + sum_a ( w_{W+K+2a} bq_a(z) + w_{W+K+2a+1} wq_a(z) ) = sum_j z^(j n) s_j;
 *   permutation: bq_a = (a_a - 1) / (z - tau), wq_a = (b_a g_R(z) - a_a g_L(z)) / (z^n - tau^n); lookup: bq_a = a_a / (z - tau),
 *   wq_a = ((b_a - a_a) f_L f_T - S_a f_T + M S_b f_L) / (z^n - tau^n); g_L, g_R, f_L, f_T, S, M as in "Argument list with
 *   selectors and periodic members" with their operands at z: trace operand c is u_c, periodic operand j is pi_j(z), M is
 *   u_{mult_col}.  No denominator vanishes for z outside F_p.  Q(x_a) and Q(x_b) are recomputed from the three opened rows
 *   against the layer-0 triple.  A proof of smi_dev_air_prove_xargs or smi_dev_air_prove_deep is rejected here, and a
 *   proof of this variant by their verifiers.
 * The prover does not refuse a column that does not close: *closes is the mask of the list provers, and the verifier
 *   rejects such a proof on the consistency check.  A zero denominator in a column is SMI_ERR_NO_INVERSE as
 *   smi_dev_xargs_columns reports it.
 * Soundness accounting: DESIGN.md section 11.
 * Left out: folding factor 4 (it comes with coset leaves, below); the single permutation / lookup forms (a one-element list covers them);
 *   smi_mgpu_* twins; zero-knowledge randomisers; fusing the auxiliary quotients or the segment extension into
 *   other launches. */
/* Host only: the plan above -> d and D.  `xargs` is a pointer to an smi_air_xargs. */
int smi_air_plan_deep_xargs(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint32_t *degree, uint32_t *segments);
/* Host only: the plan, and the length in bytes of the proof of that shape (num_colinearity_tests is read as well). */
int smi_air_deep_xargs_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, size_t *proof_len);
/* The DEEP codeword of step 9 on its own: smi_dev_deep_compose with n_args auxiliary F_q columns, 1 .. SMI_ARGS_MAX.
 * d_c_lde: their 4 n_args extended coordinate columns c_stride apart (column 4 a + e = coordinate e of c_a); ood: the
 * record's 4 (2 W + 2 A + D) canonical values; challenges: as many unreduced u64 in record order.  One streaming launch,
 * 4 (W + 4 A + 4 D) + 16 bytes a point; an auxiliary column costs four loads and two prepared F_q multiplies a point.
 * 16-byte accesses when the four bases are 16-byte aligned and the four strides multiples of 4, 4-byte accesses with the
 * same values otherwise. */
int smi_dev_deep_compose_args(smi_ctx *ctx, const smi_stark_cfg *cfg, uint32_t n_args, uint32_t n_segments, const uint32_t *d_lde, size_t stride,
                              const uint32_t *d_c_lde, size_t c_stride, const uint32_t *d_seg, size_t seg_stride, const uint64_t z[4], const uint64_t *ood,
                              const uint64_t *challenges, uint32_t *d_out, size_t out_stride);
/* The prover above.  roots (optional): root_1, root_2, root_3, 96 bytes; ood (optional): the record's 4 (2 W + 2 A + D)
 * values; stage_ms (optional) gets eight values {lde, commit, args, compose, segments, ood, fri, open}; *closes (optional):
 * bit a is set iff argument a closes. */
int smi_dev_air_prove_deep_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint32_t *d_trace_cols, uint8_t *roots,
                                 uint64_t *ood, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits,
                                 uint32_t *closes);
int smi_air_verify_deep_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint8_t *roots, const uint8_t *proof,
                              size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- Out-of-domain sampling over coset leaves ---------------------------------------------------------------------------
 * The two DEEP proofs above with FRI at folding factor 4 and every committed group of columns a tree of coset leaves.  FRI
 * only sees the DEEP codeword Q, so folding it by 4 does not depend on the statement; and DEEP has no + B rows, so a test
 * needs exactly the four points of one layer-0 coset from every group -- one leaf of smi_dev_merkle_build_cosets and one
 * path of log2 N - 2 digests per tree, where a row tree would open four rows with four full paths.
 * Plans: smi_air_plan_deep and smi_air_plan_deep_xargs as they are (4 D <= 64 is the bound 16 D <= 256 of a coset leaf).
 * Prover.  Every step of "Out-of-domain sampling" (smi_dev_air_prove_deep_fold4) or of "Out-of-domain sampling with an
 * argument list" (smi_dev_air_prove_deep_xargs_fold4) applies word for word, with three differences:
 *   - every commitment is smi_dev_merkle_build_cosets over the same columns: the trace (V = W), the auxiliary coordinate
 *     columns (V = 4 A, lists only), the segments (V = 4 D).  The transcript keeps its shape -- the same objects under the
 *     same counters --; only the root values differ;
 *   - FRI is "Extension FRI, folding factor 4", continuing that transcript at E = B over Q where it stands (stride == N, no
 *     compaction copy); the nonce record is always present;
 *   - openings, after the FRI objects, one section per group in the order trace, (auxiliary,) segments, each laid out like
 *     a fold-by-4 FRI layer: t tag-2 records of 4 V values in leaf order (value 4 c + j = column c at a + j N / 4,
 *     a = top mod N / 4), then t tag-3 paths of log2 N - 2 digests.  One launch (coset_open_kernel) writes them all.
 * Proof bytes (smi_air_deep_fold4_layout, smi_air_deep_xargs_fold4_layout; len_FRI4 is smi_fri_fold4_layout's):
 *   9 + 32 (2W + D) + len_FRI4(N, B, t) + sum over V in {W, 4D} of [ t (9 + 32 V) + t (9 + 32 (log2 N - 2)) ]
 *   and with a list  9 + 32 (2W + 2A + D) + len_FRI4(N, B, t) + the same sum over V in {W, 4A, 4D}.
 * A shape without a fold (F = 0 in smi_fri_fold4_layout's count) has no layer-0 coset to compare Q with: the prover refuses
 *   it with SMI_ERR_BAD_ARG and a sentence that starts "deep fold4: FRI has no fold", and the verifier rejects every proof
 *   with the same sentence after the consistency check.  The layout functions still report folds = 0 and the length.
 * Verifier (host), in this order: the checks of smi_air_verify_deep (smi_air_verify_deep_xargs) in their order with their
 *   sentences up to and including the consistency check at z; the fold-by-4 FRI walk with the proof of work, which hands
 *   out the layer-0 coset records; the exact length of the opening sections; the tag and count of every record and path,
 *   group by group; every record hashed as it stands to its leaf and its path checked against the group's root at index a;
 *   canonical values; Q recomputed at the four points x_a iota^j, iota = omega_N^(N/4) -- group column c at point j is
 *   record value 4 c + j -- and each coordinate e compared with value 4 e + j of the test's layer-0 coset record.  The
 *   sentences of the opening checks start "deep coset openings:" ("deep argument coset openings:" with a list).  A proof of
 *   smi_dev_air_prove_deep, smi_dev_air_prove_deep_xargs or smi_dev_air_prove_ext_fold4 is rejected here, and a proof of
 *   this variant by their verifiers.
 * Soundness is that of the two sections above: a query is still worth log2 B bits.
 * Left out: the single permutation() / lookup() forms (a one-element list covers them); column trees; smi_mgpu_* twins;
 *   folding factors above 4; fusing the DEEP codeword or the fold into a leaf launch; zero-knowledge randomisers; an AIR
 *   digest in the transcript. */
/* Host only: the plan of smi_air_plan_deep, then *folds = F and the proof length in bytes (num_colinearity_tests is read). */
int smi_air_deep_fold4_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint64_t *folds, size_t *proof_len);
/* smi_dev_air_prove_deep's parameters: roots (optional) root_1, root_2, 64 bytes; stage_ms (optional) seven values
 * {lde, commit, compose, segments, ood, fri, open}. */
int smi_dev_air_prove_deep_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t *roots, uint64_t *ood,
                                 uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits);
int smi_air_verify_deep_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t *roots, const uint8_t *proof, size_t proof_len,
                              int *accept, uint32_t grind_bits);
/* The same for an argument list: the plan of smi_air_plan_deep_xargs; three roots, 96 bytes; eight stages {lde, commit,
 * args, compose, segments, ood, fri, open}; *closes as in smi_dev_air_prove_deep_xargs. */
int smi_air_deep_xargs_fold4_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint64_t *folds, size_t *proof_len);
int smi_dev_air_prove_deep_xargs_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint32_t *d_trace_cols,
                                       uint8_t *roots, uint64_t *ood, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms,
                                       uint32_t grind_bits, uint32_t *closes);
int smi_air_verify_deep_xargs_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint8_t *roots, const uint8_t *proof,
                                    size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- Zero-knowledge DEEP proofs ----------------------------------------------------------------------------------------
 * None of the proofs above hides the trace: opened rows are raw values of the trace polynomials, digests are unsalted, and
 * the segments and every FRI layer are functions of the witness.  A zero-knowledge variant of "Out-of-domain sampling over
 * coset leaves" needs randomness inside the committed polynomials, a different split of the composition, one more polynomial
 * in FRI and salted leaves.  This section adds that variant and the parts it is made of: the device random generator, the
 * plan over the derived AIR, and the masked split.  Notation is that of "Out-of-domain sampling"; t = the number of
 * colinearity tests, and a test opens one layer-0 coset of 4 points.
 * Random residues (smi_dev_random_fill).  The project's 32-byte hash in counter mode.  Element i of a stream is
 *     u64_le(digest[8 k .. 8 k + 7]) mod p,  k = i mod 4,  digest = Hash::from_bytes(message),  message (48 bytes) =
 *     seed[0 .. 31] | stream_id as 8 little-endian bytes | floor(i / 4) as 8 little-endian bytes.
 *   p < 2^30 and the word is uniform on 2^64 values, so an element's bias is below p / 2^64 < 2^-34.  Streams with different
 *   stream_id, or different seeds, are independent under the random-oracle reading of the hash; the same (seed, stream_id,
 *   count) gives the same words on every call, whatever the alignment of d_out.  One launch, no atomics: a lane hashes the
 *   counters 2 l and 2 l + 1 the way the grinding search hashes transcript | nonce (the 40 leading bytes travel as a
 *   midstate) and stores elements 8 l .. 8 l + 7 with two 16-byte stores when d_out is 16-byte aligned.
 * Trace randomisers and the derived AIR (smi_air_plan_deep_zk).  k_t = 8 t + 8.  The statement covers the first n - k_t
 *   rows; a prover overwrites the last k_t rows of every trace column with random residues, which makes k_t off-domain
 *   functionals of f_c jointly uniform: f_c at the 4 t queried points, f_c at w times those points (through H), and f_c(z),
 *   f_c(z w), four base-field functionals each.  Transitions are exempt on rows n - k_t - 1 .. n - 2 (row n - 1 already is)
 *   without a new composition kernel: the library derives an AIR that differs from the caller's in one more periodic column
 *   of period n, index Q, holding E(tau w^r) for E(x) = prod_{r = n - k_t - 1}^{n - 2} (x - tau w^r), and in every term of
 *   every transition constraint carrying that column as one more factor (variables 2 W + Q + j move up by one).  The
 *   interpolant of those n values is E itself, of degree k_t, so smi_dev_air_compose_ext, the periodic tables and a verifier's
 *   pi_j(z) do the work unchanged, and the derived AIR holds on every row pair of an honest trace whatever the tail holds.
 *   d and D are smi_air_plan_deep's for the derived AIR: a periodic factor is charged like a column, which is what the
 *   true degree (d - 1) n + k_t needs once D is a power of two.
 * Masked segments (smi_dev_zk_segments).  H_j(x_i) one by one is a global function of the witness, so the split changes:
 *   k_s = 4 t + 1 (a segment is opened at 4 t points and at z), L = n - k_s, D' = ceil(D n / L), 4 D' + 5 <= 64 (the
 *   segments, four mask columns and a salt column in one coset leaf).  From the 4 coefficient columns of H one streaming
 *   launch writes 4 D' columns of exactly n coefficients, column 4 j + e = coordinate e of
 *     H~_j[m]     = H[j L + m] - rho_{j-1}[m]   for m < L   (the rho term for m < k_s only; H reads 0 at and above h_len)
 *     H~_j[L + m] = rho_j[m]                    for m < k_s
 *   with rho_{-1} = rho_{D'-1} = 0 and rho_j (j < D' - 1) k_s coefficients of F_q, coordinate e of rho_j at
 *   d_rho[(4 j + e) k_s ..].  Then sum_j x^{j L} H~_j = H identically, every H~_j has degree < n, and any D' - 1 of them at
 *   k_s points are uniform.  16-byte accesses when d_h and d_out are 16-byte aligned and both strides are multiples of 4,
 *   4-byte accesses with the same values otherwise.
 * Refused by the plan with SMI_ERR_BAD_ARG and a sentence (smi_air_last_error) that starts "zk deep:": k_t >= n / 2; a
 *   boundary point on a row >= n - k_t; 4 D' + 5 > 64; W + 1 > 64 (the trace tree's salt column); and whatever
 *   smi_air_plan_deep refuses for the derived AIR, in its words.
 * The proof (smi_dev_air_prove_deep_zk, smi_air_verify_deep_zk).  "Out-of-domain sampling over coset leaves" for a plain AIR
 *   with D -> D' and:
 *   - random values.  Everything comes from smi_dev_random_fill under the caller's seed, so a proof is a pure function of
 *     (trace, seed); the seed is never part of a proof.  Streams: 1 = the randomiser rows (column c takes elements
 *     c k_t .. (c + 1) k_t - 1 in its rows n - k_t .. n - 1; d_trace_cols is overwritten IN PLACE, as
 *     smi_dev_lookup_multiplicities writes in place), 2 = the salt column of tree 1 (N residues), 3 = rho (4 (D' - 1) k_s),
 *     4 = the mask R (coordinate e takes elements e n .. (e + 1) n - 1 as its n coefficients), 5 = the salt column of tree 2;
 *   - tree 1 is smi_dev_merkle_build_cosets over the W extended trace columns and the salt column (W + 1 <= 64); tree 2 over
 *     the 4 D' extended segment columns, the 4 extended columns of R and the salt column.  A salt column is N raw residues,
 *     no codeword: 4 salt values, about 120 bits, in every leaf;
 *   - the transcript keeps the DEEP shape: root_1, the composition weights, root_2, z, the record of 4 (2 W + D') values
 *     (u, v, s_j = H~_j(z)), as many gammas, fold-by-4 FRI with the nonce record.  R has no DEEP quotient and is not opened
 *     at z;
 *   - FRI runs on Q' = Q + R, Q = smi_dev_deep_compose with D' segments; R is added by one small streaming launch
 *     (zk_mask_add_kernel) after the DEEP compose launch, which stays as it is;
 *   - the opening sections hold records of 4 (W + 1) and 4 (4 D' + 5) values.
 * Proof bytes (smi_air_deep_zk_layout): 9 + 32 (2 W + D') + len_FRI4(N, B, t) + sum over V in {W + 1, 4 D' + 5} of
 *   [ t (9 + 32 V) + t (9 + 32 (log2 N - 2)) ].
 * Verifier (host), in this order, every sentence starting "zk deep": the record's tag and count; canonical coordinates; z
 *   outside the base field; the consistency check -- the left side of smi_air_verify_deep's over the DERIVED AIR (the
 *   exemption column evaluated at z and z w like any periodic column) against sum_j z^(j L) s_j; a shape without a fold; the
 *   fold-by-4 FRI walk; the sections' exact length, tags and counts; every record hashed as it stands (salts included) and
 *   its path; canonical values (the salts are not looked at); Q + R recomputed at the four coset points against the
 *   layer-0 record.  A proof of smi_dev_air_prove_deep_fold4 is rejected here and a proof of this variant by
 *   smi_air_verify_deep_fold4: their records differ in length (D' > D).
 * Left out: row leaves / fold 2; smi_mgpu_* twins; an AIR digest in the transcript.  Argument lists: the next section. */
/* Host only: *degree = d and *segments = D' for the derived AIR, *k_t and *k_s for cfg->num_colinearity_tests (outputs are
 * optional). */
int smi_air_plan_deep_zk(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint32_t *degree, uint32_t *segments, uint32_t *k_t, uint32_t *k_s);
/* d_out: count u32 residues (count <= 2^34).  Asynchronous on the context's stream. */
int smi_dev_random_fill(smi_ctx *ctx, const uint8_t seed[32], uint64_t stream_id, uint32_t *d_out, size_t count);
/* d_h: coordinate e of H's coefficients at d_h + e h_stride, h_len <= D' (n - k_s) of them; d_rho: 4 (D' - 1) k_s words (may
 * be null when n_segments == 1); d_out: column c at d_out + c out_stride, out_stride >= n = 2^log_n.  log_n in 2 .. 27,
 * 1 <= k_s < n / 2, 1 <= n_segments <= 14.  Asynchronous on the context's stream. */
int smi_dev_zk_segments(smi_ctx *ctx, const uint32_t *d_h, size_t h_stride, size_t h_len, uint32_t log_n, uint32_t k_s, uint32_t n_segments,
                        const uint32_t *d_rho, uint32_t *d_out, size_t out_stride);
/* Host only: the plan above, then *folds = F and the proof length in bytes. */
int smi_air_deep_zk_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint64_t *folds, size_t *proof_len);
/* smi_dev_air_prove_deep_fold4's parameters with the seed; d_trace_cols is overwritten in its last k_t rows; roots (optional)
 * root_1, root_2, 64 bytes; stage_ms (optional) nine values {random, lde, commit, compose, segments, ood, mask, fri, open}.
 */
int smi_dev_air_prove_deep_zk(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, uint32_t *d_trace_cols, const uint8_t seed[32], uint8_t *roots,
                              uint64_t *ood, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits);
int smi_air_verify_deep_zk(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t *roots, const uint8_t *proof, size_t proof_len,
                           int *accept, uint32_t grind_bits);

/* ---- Zero-knowledge DEEP proofs with an argument list -------------------------------------------------------------------
 * The zero-knowledge variant of "Out-of-domain sampling over coset leaves" for an smi_air_xargs list (FRI folding factor 4).
 * Notation is that of "Zero-knowledge DEEP proofs" and of "Out-of-domain sampling with an argument list"; the recurrences,
 * T_a and init_a (1 for a permutation, 0 for a lookup) are those of "Argument list with selectors and periodic members".
 * The plain variant cannot simply derive a list: an auxiliary column c_a wraps around over all n rows, is a deterministic
 * function of the trace and two challenges, and is opened at the queried points, at z and at z w.  So c_a gets randomiser
 * rows of its own, a transition that is exempt on them, and a closing condition that no longer rests on the wrap.
 * Rows.  k_t = 8 t + 16 (the plain variant keeps 8 t + 8), k_s = 4 t + 1, n_a = n - k_t active rows.  The statement covers
 *   the main transitions on the row pairs (r, r + 1), r <= n_a - 2, boundary points on rows < n_a, and every argument over
 *   the rows < n_a only.  Why 16: a coordinate column of c_a has k_t - 1 free rows (below) and is revealed through 8 t + 8
 *   base-field functionals -- 4 t queried points, 4 t points w x through H, and z and z w, four each.
 * Trace randomisers.  Stream 1, the last k_t rows of every trace column, written in place BEFORE the auxiliary columns are
 *   built (column c takes elements c k_t .. (c + 1) k_t - 1).
 * Derived AIR (smi_air_plan_deep_zk_xargs).  The caller's AIR with two more periodic columns of period n.  Index Q holds
 *   E(tau w^r), E(x) = prod_{r = n_a - 1}^{n - 2} (x - tau w^r), a factor of every term of every transition constraint, exactly
 *   as in the plain variant with this k_t.  Index Q + 1 holds E_A(tau w^r), E_A(x) = prod_{r = n_a}^{n - 1} (x - tau w^r); no
 *   main constraint reads it.  Variables 2 W + Q + j move up by two.  Refused when Q + 2 > SMI_AIR_MAX_PERIODIC.
 * Auxiliary columns (smi_dev_zk_args_tail).  c_a[0] = init_a, and c_a[r + 1] follows from c_a[r] by the recurrence for r < n_a,
 *   so c_a[n_a] is the closing value: argument a closes iff c_a[n_a] = init_a.  Rows n_a + 1 .. n - 1 of the four coordinate
 *   columns of c_a are random: coordinate column 4 a + e takes elements (4 a + e)(k_t - 1) .. of stream 6.  The three-launch
 *   column build runs over all n rows of the randomised trace -- its rows <= n_a are already right, and n_a is a multiple of
 *   8, so no lane mixes active and tail rows; one more launch (zk_args_tail_kernel) then copies c_a[n_a] into the verdict
 *   flags and overwrites the tail, with 16-byte stores where the alignment allows (n_a + 1 is odd: the head of every column's
 *   tail is unaligned) and 4-byte stores of the same words otherwise.  *closes bit a is that verdict; the prover does not
 *   refuse a column that does not close.  A zero denominator in any of the n rows is reported as smi_dev_xargs_columns
 *   reports it.
 * Auxiliary quotients (smi_dev_air_compose_zk_xargs).  Three per argument, under the weights w_{W+K+3a}, w_{W+K+3a+1},
 *   w_{W+K+3a+2}, so NW = W + K + 3 A:
 *     bq_a = (c_a(x) - init_a) / (x - tau)
 *     wq_a = E_A(x) T_a(x) / (x^n - tau^n)        T_a: the wrapping transition numerator of the xargs section, unchanged
 *     cq_a = (c_a(x) - init_a) / (x - tau w^n_a)
 *   E_A(x_i) is read from the derived AIR's extended periodic table Q + 1 the way a periodic operand is read.  One streaming
 *   launch after smi_dev_air_compose_ext; the eight denominators x - tau, x - tau w^n_a of a lane's four points share one
 *   inversion whatever A is.
 * Degree.  An argument contributes one more than in the xargs section: a permutation 3, with a selector 4, a lookup 4;
 *   d = max(d of the derived AIR, contributions); D, D' = ceil(D n / (n - k_s)), D <= B, 4 D' + 5 <= 64, W + 1 <= 64 and
 *   k_t < n / 2 as in the plain zk plan; no boundary point on a row >= n_a.  Refusals start "zk deep argument:".
 * Multiplicities (smi_dev_xargs_multiplicities_rows).  smi_dev_xargs_multiplicities with a row bound: table rows >= rows are
 *   not inserted, lookup rows >= rows are not counted, the column stride stays n; rows = n gives every word of that call.  A
 *   caller fills the multiplicity columns with rows = n_a before the randomiser rows are written.
 * Trees (coset leaves).  Tree 1: W + 1 columns (salt: stream 2).  Tree 2: 4 A + 1 (salt: stream 7).  Tree 3: 4 D' + 5, the
 *   segments, the mask R and a salt (stream 5).  Streams 3 (rho) and 4 (R) as in the plain variant.
 * Transcript and record.  The shape of "Out-of-domain sampling with an argument list" with NW above: root_1 -> alpha, gamma;
 *   root_2 -> 4 NW weights; root_3 -> z; the record of 4 (2 W + 2 A + D') values u, v, a_a, b_a, s_j = H~_j(z); as many
 *   gammas.  R has no DEEP quotient.
 * Codeword.  Q' = Q + R: smi_dev_deep_compose_args with D' segments, then zk_mask_add_kernel.  Fold-by-4 FRI with the nonce
 *   record.
 * Proof bytes (smi_air_deep_zk_xargs_layout): 9 + 32 (2 W + 2 A + D') + len_FRI4(N, B, t) + sum over V in {W + 1, 4 A + 1,
 *   4 D' + 5} of [ t (9 + 32 V) + t (9 + 32 (log2 N - 2)) ].
 * Verifier (host), every sentence starting "zk deep argument", in the order of smi_air_verify_deep_zk over three sections.
 *   The consistency check is
 *     sum_c w_c term_c(z) + sum_k w_{W+k} tq_k(z) + sum_a (w bq_a(z) + w wq_a(z) + w cq_a(z)) = sum_j z^(j L) s_j
 *   over the derived AIR; wq_a carries E_A(z), cq_a = (a_a - init_a) / (z - tau w^n_a), the operands at z are those of
 *   smi_air_verify_deep_xargs.  Q + R is recomputed at the four coset points from the three opened records.  Proofs of
 *   smi_dev_air_prove_deep_xargs_fold4 and of smi_dev_air_prove_deep_zk are rejected here, and this variant's proofs by their
 *   verifiers: the records differ in length.
 * Measured (profiles/zk_args_time.log): the 9-column list of README.md at n = 2^20, B = 8, t = 32, 16 grinding bits -- 1.36 times
 *   the stage time of smi_dev_air_prove_deep_xargs_fold4 (wall time 1.93 times), proof 1.08 times its bytes.
 * Left out: row leaves / fold 2; the single permutation and lookup forms (a one-element list covers them); smi_mgpu_* twins;
 *   next-row operands (SMI_ARG_NEXT_ROW: the row after the last active row is random, and the statement over the active rows
 *   needs a decision of its own -- the plan refuses such a list); an AIR digest in the transcript. */
/* Host only: *degree = d, *segments = D', *k_t = 8 t + 16, *k_s (outputs are optional). */
int smi_air_plan_deep_zk_xargs(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint32_t *degree, uint32_t *segments, uint32_t *k_t,
                               uint32_t *k_s);
/* Host only: the plan above, then *folds = F and the proof length in bytes. */
int smi_air_deep_zk_xargs_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint64_t *folds, size_t *proof_len);
/* smi_dev_xargs_multiplicities over the rows < rows (1 <= rows <= n); all n words of d_mult are written. */
int smi_dev_xargs_multiplicities_rows(smi_ctx *ctx, const void *air, const void *xargs, uint32_t a, const uint32_t *d_trace_cols, uint32_t n_cols,
                                      uint32_t log_n, size_t rows, uint32_t *d_mult);
/* The tail step alone.  d_c: 4 n_args coordinate columns of n = 2^log_n words, c_stride >= n apart; k_t a multiple of 8 below
 * n / 2; d_rnd: 4 n_args (k_t - 1) words.  closing (optional, host): 4 n_args values, coordinate e of c_a[n - k_t] at 4 a + e;
 * the call synchronises when it is given. */
int smi_dev_zk_args_tail(smi_ctx *ctx, uint32_t *d_c, size_t c_stride, uint32_t log_n, uint32_t k_t, uint32_t n_args, const uint32_t *d_rnd,
                         uint64_t *closing);
/* smi_dev_air_compose_xargs's parameters: the composition of the DERIVED AIR plus the 3 A auxiliary quotients; d_weights:
 * 4 (W + K + 3 A) unreduced coordinates on the device. */
int smi_dev_air_compose_zk_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint32_t *d_lde, size_t stride,
                                 const uint32_t *d_c_lde, size_t c_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                                 size_t out_stride);
/* smi_dev_air_prove_deep_zk's parameters with the list; roots (optional) root_1, root_2, root_3, 96 bytes; stage_ms (optional)
 * ten values {random, lde, commit, args, compose, segments, ood, mask, fri, open}; *closes as in smi_dev_air_prove_deep_xargs. */
int smi_dev_air_prove_deep_zk_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint32_t *d_trace_cols,
                                    const uint8_t seed[32], uint8_t *roots, uint64_t *ood, uint8_t **proof, size_t *proof_len, uint64_t *top_indices,
                                    double *stage_ms, uint32_t grind_bits, uint32_t *closes);
int smi_air_verify_deep_zk_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint8_t *roots, const uint8_t *proof,
                                 size_t proof_len, int *accept, uint32_t grind_bits);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ---------------------------
 * Fri::commit / Fri::prove (src/fri.rs:105-156, 250-311) over ONE codeword sharded in contiguous
 * blocks (rank g holds [g*N/G, (g+1)*N/G)), and the build-defined trace -> proof composition of
 * smi_dev_stark_prove over the G ranks.  Every rank makes the same calls in the same order; the
 * collectives (all-gather of the G sub-roots per tree, one grouped send/recv per fold and for the
 * extension's all-to-all, one byte-sum all-reduce of the proof) run inside the library on the
 * context's stream.  Results are bit-identical to the single-GPU entry points by construction and
 * as far as they have been run: at every world size (2, 4, 8) on the CPU instantiation of the same loop,
 * with 2 and 4 ranks on one GPU through smi_mgpu_create_with (host-staged collectives), and over a real
 * RCCL communicator at world size 1.  An RCCL communicator with MORE THAN ONE RANK has not been exercised:
 * the development boxes have one GPU.  bench.py therefore self-checks three entry points against their
 * single-GPU twins on every rank before it times anything on several GPUs.  World sizes are powers of two. */
typedef struct smi_mgpu smi_mgpu;
#define SMI_MGPU_ID_BYTES 128
/* rank 0: ncclGetUniqueId; the caller carries the 128 bytes to the other ranks (any channel) */
int smi_mgpu_unique_id(uint8_t id[SMI_MGPU_ID_BYTES]);
/* ncclCommInitRank on the context's device; collective over all ranks */
int smi_mgpu_create(smi_ctx *ctx, const uint8_t id[SMI_MGPU_ID_BYTES], int rank, int world, smi_mgpu **out);
/* The same prover over caller-supplied collectives (tests without several GPUs, other transports).
 * Pointers are device memory; the library drains its stream before each call and expects the
 * operation to have completed on return (0 = ok).  exchange: the k-th send to a peer matches that
 * peer's k-th recv from this rank. */
typedef struct {
    void *user;
    int (*all_gather)(void *user, const void *d_send, void *d_recv, size_t bytes_per_rank);
    int (*exchange)(void *user, int n_send, const int *send_peer, void *const *d_send, const size_t *send_bytes, int n_recv,
                    const int *recv_peer, void *const *d_recv, const size_t *recv_bytes);
    int (*all_reduce_sum_u8)(void *user, void *d_buf, size_t bytes);
} smi_mgpu_coll;
int smi_mgpu_create_with(smi_ctx *ctx, const smi_mgpu_coll *ops, int rank, int world, smi_mgpu **out);
void smi_mgpu_destroy(smi_mgpu *m);
/* blocks shorter than this are all-gathered and the remaining rounds run replicated (default 2^18) */
int smi_mgpu_set_min_block(smi_mgpu *m, size_t min_block);
/* Fri::commit: d_block = this rank's block of the initial codeword (device u32).  roots: R x 32,
 * alphas: R-1 unreduced u64, last codeword as u64 -- on every rank. */
int smi_mgpu_fri_commit(smi_mgpu *m, const smi_fri_cfg *cfg, const uint32_t *d_block, size_t block_len, uint8_t *roots, uint64_t *alphas,
                        uint64_t *last_codeword, size_t *last_len);
/* Fri::prove: the serialized ProofStream (smi_free) and the top-level indices on every rank. */
int smi_mgpu_fri_prove(smi_mgpu *m, const smi_fri_cfg *cfg, const uint32_t *d_block, size_t block_len, uint8_t **proof, size_t *proof_len,
                       uint64_t *top_indices);
/* The same two continuing the caller's FiatShamir (Fri::commit / Fri::prove, src/fri.rs:105-156, 250-311, as
 * smi_fri_commit_fs / smi_fri_prove_fs): transcript = host bytes, the same on every rank; the proof is what the
 * method pushes after the caller's objects. */
int smi_mgpu_fri_commit_fs(smi_mgpu *m, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_block,
                           size_t block_len, uint8_t *roots, uint64_t *alphas, uint64_t *last_codeword, size_t *last_len);
int smi_mgpu_fri_prove_fs(smi_mgpu *m, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_block,
                          size_t block_len, uint8_t **proof, size_t *proof_len, uint64_t *top_indices);
/* The extension of smi_dev_lde sharded by (column, coset) units (n_cols << log_blowup and 2^log_n
 * multiples of the world size, log_blowup <= 4): d_trace_cols = the whole trace on every rank;
 * d_out_blocks gets this rank's natural-order block of every column (n_cols x N/G, stride N/G). */
int smi_mgpu_lde(smi_mgpu *m, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, uint32_t log_blowup, uint64_t trace_offset,
                 uint64_t lde_offset, uint32_t *d_out_blocks);
/* ONE transform of 2^log_n points over the G ranks (BASELINE configs[3]; the reference has no NTT, this is
 * Polynomial::eval_domain / interpolate_domain on a geometric domain of that size, src/univariate/eval.rs:16-21,
 * interpolate.rs:6-44) on the ordinary pass pipeline with ONE all-to-all.  With R_0 = 2^*log_r0 the
 * plan's first digit (smi_mgpu_ntt_first_digit) and B = N / R_0:
 *   d_strip: this rank's columns [rank*B/G, (rank+1)*B/G) of the row-major [R_0][B] view of the input, as
 *            [R_0][B/G] (clobbered);
 *   d_out  : N/G outputs, X[k_0 + R_0*rest] at rest*(R_0/G) + (k_0 - rank*R_0/G) -- natural-order runs of R_0/G.
 * Forward: evaluations on offset*<w_N>; inverse (offset must be 1): coefficients from values.  At G = 1 it is
 * the direct transform. */
int smi_mgpu_ntt(smi_mgpu *m, uint32_t *d_strip, uint32_t *d_out, uint32_t log_n, int inverse, uint64_t offset);
/* The same transform with the result as this rank's CONTIGUOUS natural-order block: d_out gets X[rank*N/G ..
 * (rank+1)*N/G), the layout smi_mgpu_fri_commit / smi_mgpu_fri_prove take (so a 2^26-point evaluation can be
 * committed without leaving the GPUs).  Costs a second all-to-all of the same volume: with one exchange the rank
 * that owns k_0 holds every R_0-th output, and a contiguous output range is a range of the other index. */
int smi_mgpu_ntt_natural(smi_mgpu *m, uint32_t *d_strip, uint32_t *d_out, uint32_t log_n, int inverse, uint64_t offset);
int smi_mgpu_ntt_first_digit(uint32_t log_n, uint32_t *log_r0);
/* smi_dev_stark_prove (column trees) over the G ranks: same column roots, same proof bytes. */
int smi_mgpu_stark_prove(smi_mgpu *m, const smi_stark_cfg *cfg, const uint32_t *d_trace_cols, uint8_t *column_roots, uint8_t **proof,
                         size_t *proof_len, uint64_t *top_indices);

#ifdef __cplusplus
}
#endif
#endif /* STARK_MI_H */
