// internal.h -- context and helpers shared by the translation units of libstarkmi.so.
#pragma once
#include <string.h>
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/stark_mi.h"
#include "fri_plan.h"
#include "tables.h"
#include "transcript_core.h"

struct ScaleEntry {
    uint32_t c, q, L;
    uint32_t *lo, *hi;
    uint64_t epoch;   // smi_ctx::scale_epoch of the last ScaleScope that looked it up (pinned while that scope is open)
};

struct ProfRec {
    const char *name;
    hipEvent_t e0, e1;
    double bytes;
    double mixes;   // hash kernels: mix_state evaluations of the launch (smi_kernel_time::alg_mixes)
};

struct smi_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    FieldSetup fs;
    uint32_t *d_tab[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};  // [dir][tw10, lo, hi]
    std::vector<ScaleEntry> scale_cache;
    uint64_t scale_epoch = 1;   // bumped when an outermost ScaleScope opens
    int scale_depth = 0;        // open ScaleScopes (they nest: stark_prove -> fri_run -> fold)
    uint32_t *d_root_tab[32] = {};   // [log m]: w_m^e, e < m, as (value, Shoup quotient) pairs (ctx_root_table)
    uint32_t *scratch = nullptr;   // NTT inter-pass buffer
    size_t scratch_elems = 0;
    void *tmp[4] = {nullptr, nullptr, nullptr, nullptr};  // staging buffers of the host-buffer entry points
    size_t tmp_bytes[4] = {0, 0, 0, 0};
    int *d_flag = nullptr;         // non-canonical input flag
    void *pin[2] = {nullptr, nullptr};          // pinned chunks of the large host <-> device transfers
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    void *pin_out = nullptr;       // pinned landing buffer of a prove's results (proof bytes, challenges, indices, roots)
    size_t pin_out_bytes = 0;
    std::string err;
    bool prof_on = false;
    char prof_only[56] = {0};   // smi_ctx_profile_only: bracket only launches whose name contains this (empty: all)
    bool copy_probe = false;       // smi_ctx_copy_probe: NTT passes launch their copy-only twins
    // three-pass transforms: the second pass applies the first pass's inter-pass twiddle as it loads (ntt_core.h)
    // tuning knob, default 1: 0 never, 1 the launchers' rule (NttPass::share_cols), 2 whenever the pass has multipliers (no
    // launch-size threshold: how the tests reach the column-sharing kernels at small sizes); any other value is 1
    int ntt_share_cols = !getenv("SMI_NTT_SHARE_COLS") ? 1 : atoi(getenv("SMI_NTT_SHARE_COLS")) == 0 ? 0 : atoi(getenv("SMI_NTT_SHARE_COLS")) == 2 ? 2 : 1;
    bool ntt_twin_regs = !(getenv("SMI_NTT_TWIN_REGS") && atoi(getenv("SMI_NTT_TWIN_REGS")) == 0);   // tuning knob, default on: deferred twiddles held as per-thread input multipliers
    bool ntt_last_direct = !(getenv("SMI_NTT_LAST_DIRECT") && atoi(getenv("SMI_NTT_LAST_DIRECT")) == 0);   // NttRequest::last_direct; tuning knob, default on
    int ntt_defer_tw = getenv("SMI_NTT_DEFER_TW") ? (atoi(getenv("SMI_NTT_DEFER_TW")) != 0) : 2;   // NttRequest::defer_tw; tuning knob, default 2 (auto)
    bool lde_two_pass = getenv("SMI_LDE_TWO_PASS") && atoi(getenv("SMI_LDE_TWO_PASS"));   // smi_ctx_lde_two_pass
    std::vector<ProfRec> prof;
    // bump arena for the per-prove device buffers (trees, folded codewords, proof bytes):
    // steady state does no hipMalloc/hipFree.  Overflow allocations are tracked and the
    // arena is regrown to the high-water mark at the next reset.
    uint8_t *arena = nullptr;
    size_t arena_size = 0, arena_used = 0, arena_want = 0;
    std::vector<void *> arena_overflow;
};
int arena_reset(smi_ctx *ctx);                       // syncs the stream if memory has to move
void *arena_alloc(smi_ctx *ctx, size_t bytes);       // nullptr on OOM

// HIP-event bracket around one kernel launch (no-ops unless profiling is enabled)
struct ProfScope {
    smi_ctx *ctx;
    ProfRec r;
    bool on;
    ProfScope(smi_ctx *c, const char *name, double bytes, double mixes = 0.0) : ctx(c), on(c->prof_on) {
        if (on && c->prof_only[0] && !strstr(name, c->prof_only)) on = false;
        if (!on) return;
        r.name = name;
        r.bytes = bytes;
        r.mixes = mixes;
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(r.e0, ctx->stream);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.e1, ctx->stream);
        ctx->prof.push_back(r);
    }
};

// A prover's stage_ms: `count` stages between count + 1 events on the context's stream.  The events exist only when the
// caller passed stage_ms (timed) and are destroyed on every return path.  HIP_TRY(ctx, timer.create()) once, mark() at each
// stage boundary in order, write(stage_ms) after the prover's final hipStreamSynchronize: exactly `count` values.
struct StageTimer {
    smi_ctx *ctx;
    std::vector<hipEvent_t> ev;   // empty when not timed
    size_t next = 0;
    StageTimer(smi_ctx *c, uint32_t count, bool timed) : ctx(c), ev(timed ? count + 1 : 0, nullptr) {}
    ~StageTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    hipError_t create() {
        for (hipEvent_t &e : ev) {
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
        }
        return hipSuccess;
    }
    void mark() {
        if (next < ev.size()) (void)hipEventRecord(ev[next++], ctx->stream);
    }
    void write(double *stage_ms) const {
        for (size_t i = 0; i + 1 < ev.size(); i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            stage_ms[i] = ms;
        }
    }
};

// Every public entry point runs on the context's device whatever the caller's current device is
// (a process may hold contexts on several GPUs, or torch may have selected another one), and
// leaves the caller's selection as it found it.
struct DeviceGuard {
    int prev = -1;
    bool moved = false;
    explicit DeviceGuard(const smi_ctx *ctx) {
        if (!ctx) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != ctx->device) moved = hipSetDevice(ctx->device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (moved) (void)hipSetDevice(prev);
    }
};

struct smi_tree {
    smi_ctx *ctx;
    uint8_t *d_nodes;   // (2n-1) x 32 bytes, level 0 first
    size_t n;
    bool owns;
};

int smi_hip_fail(smi_ctx *ctx, hipError_t e, const char *what);
#define HIP_TRY(ctx, call)                                             \
    do {                                                               \
        hipError_t e__ = (call);                                       \
        if (e__ != hipSuccess) return smi_hip_fail((ctx), e__, #call); \
    } while (0)
#define SMI_TRY(call)            \
    do {                         \
        int rc__ = (call);       \
        if (rc__ != SMI_OK) return rc__; \
    } while (0)

int smi_fail(smi_ctx *ctx, int code, const char *msg);
// a prove's serialized bytes as the C ABI hands them out: malloc'ed, the caller frees
inline int smi_proof_out(smi_ctx *ctx, const std::vector<uint8_t> &bytes, uint8_t **proof, size_t *proof_len) {
    *proof = (uint8_t *)malloc(bytes.size() ? bytes.size() : 1);
    if (!*proof) return smi_fail(ctx, SMI_ERR_OOM, "malloc proof");
    memcpy(*proof, bytes.data(), bytes.size());
    *proof_len = bytes.size();
    return SMI_OK;
}

// grows (never shrinks) a context-owned staging buffer
int ctx_tmp(smi_ctx *ctx, int slot, size_t bytes, void **out);
int ctx_scratch(smi_ctx *ctx, size_t elems, uint32_t **out);
// Pinned host memory for the results a prove copies back (grows, never shrinks): a device-to-host copy into pageable
// memory is staged and blocks per call (r03 trace: 6 copies, 105 us of idle at the end of a prove); into pinned
// memory the copies queue behind the last kernel and one synchronisation waits for all of them.
int ctx_pin_out(smi_ctx *ctx, size_t bytes, uint8_t **out);
NttTables ctx_tables(const smi_ctx *ctx, int inverse);
// device tables of c * q^i, i < 2^L (cached per (c,q,L))
// device table of w_m^e, e < m = 2^log_m (forward root), as Tw2 pairs; cached per log_m (log_m <= 17)
int ctx_root_table(smi_ctx *ctx, uint32_t log_m, const Tw2 **out);
int ctx_scale_tables(smi_ctx *ctx, uint32_t c_plain, uint32_t q_plain, uint32_t L, ScaleTables *out);
#define SMI_SCALE_CACHE_MAX 96   // soft cap: entries pinned by an open ScaleScope are never evicted, the cache grows instead
int ctx_scale_reserve(smi_ctx *ctx, size_t n);   // room for n more entries (evicts unpinned ones only)
// Pins every scale table looked up while it is open: ctx_scale_tables hands out raw device pointers, and a caller
// that holds one (or collects several, like the fused FRI tail) across another lookup must not see it freed by
// that lookup's eviction.  Open one in every function that takes tables and enqueues the launches that read
// them; an eviction drains the stream before it frees, so a table is safe once its launch is enqueued.
struct ScaleScope {
    smi_ctx *c;
    explicit ScaleScope(smi_ctx *ctx) : c(ctx) {
        if (c->scale_depth++ == 0) c->scale_epoch++;
    }
    ~ScaleScope() { c->scale_depth--; }
    ScaleScope(const ScaleScope &) = delete;
    ScaleScope &operator=(const ScaleScope &) = delete;
};

// field helpers on the host (plain form)
inline uint32_t h_mul(const smi_ctx *c, uint32_t a, uint32_t b) { return host_mulmod(a, b, c->fs.F.p); }
inline uint32_t h_pow(const smi_ctx *c, uint32_t a, uint64_t e) { return host_powmod(a, e, c->fs.F.p); }
inline uint32_t h_inv(const smi_ctx *c, uint32_t a) { return host_powmod(a, c->fs.F.p - 2, c->fs.F.p); }
inline uint32_t h_root(const smi_ctx *c, uint32_t log_n) {  // primitive 2^log_n-th root (forward)
    return host_powmod(c->fs.wmax[0], 1ull << (c->fs.K - log_n), c->fs.F.p);
}

// the FRI instance of a proof over the extended trace domain (stark.hip's build-defined composition at E = the blowup,
// the AIR proofs at the E of their plan): provers and verifiers take it from here
inline smi_fri_cfg trace_fri_cfg(const smi_ctx *c, const smi_stark_cfg *cfg, uint64_t E) {
    smi_fri_cfg fc;
    fc.omega = h_root(c, cfg->log_n + cfg->log_blowup);
    fc.offset = cfg->lde_offset;
    fc.domain_length = 1ull << (cfg->log_n + cfg->log_blowup);
    fc.expansion_factor = E;
    fc.num_colinearity_tests = cfg->num_colinearity_tests;
    return fc;
}

// One launch for the last rounds of Fri::commit (hash.hip, fri_tail_kernel): round k hashes and commits
// cw (len elements), runs the Fiat-Shamir round of its root and, unless next == nullptr (the last
// round), folds into next with the round's x^-1 table S.
// (SMI_FRI_TAIL_MAX_ROUNDS, SMI_FRI_TAIL_MAX_LEN: fri_plan.h)
struct FriTailRound {
    const uint32_t *cw;
    uint32_t *next;
    uint8_t *nodes;
    uint8_t *proof_slot;
    uint64_t *alpha_out;   // nullptr on the last round
    ScaleTables S;
    uint32_t len;
};
struct FriTailArgs {
    FriTailRound r[SMI_FRI_TAIL_MAX_ROUNDS];
    uint32_t n_rounds;
    uint32_t *fs_words;
    Fp F;
    uint32_t inv2_m;
    // optional: the fold that produces r[0].cw (from the halves pre_lo / pre_hi of the round before, with its challenge
    // and x^-1 table) runs at the head of the launch instead of in a fold launch of its own; pre_lo == nullptr: it does not
    const uint32_t *pre_lo, *pre_hi;
    const uint64_t *pre_alpha;
    ScaleTables pre_S;
};
int launch_fri_tail(smi_ctx *ctx, const FriTailArgs &a);
uint64_t fri_tail_len();   // codewords of at most this many elements finish in the fused tail (SMI_FRI_TAIL, default 512; fri.hip)
inline FsSeed fresh_seed() { return fs_seed_of(nullptr, 0); }   // FsSeed: transcript_core.h

// Where the leaves of a tree come from when they are not simply read (hash.hip, merkle_sub_kernel's LEAF_* kinds): the
// kernel computes the codeword element, stores it to cw_out (the query phase and the next fold read it) and hashes it.
// The hash kernels are bound by integer issue and leave HBM idle, so the fold's / the combination's reads and writes ride
// along for the price of their few arithmetic instructions -- one launch and one pass over the codeword less per round.
//   LEAF_FOLD   : element i = Fri::fold_codeword(lo[i], hi[i]) (src/fri.rs:57-91; fri_core.h fold_element, the function the
//                 stand-alone fri_fold_kernel runs) with the round's challenge read from device memory;
//   LEAF_COMBINE: element i = sum_c (weights[c] mod p) * cols[c * stride + i] (combine_columns_kernel's sum, same order).
enum { LEAF_LOAD = 0, LEAF_FOLD = 1, LEAF_COMBINE = 2 };
#define SMI_LEAF_COMBINE_MAX 8
struct LeafSrc {
    int kind;
    uint32_t *cw_out;
    Fp F;
    // LEAF_FOLD
    const uint32_t *lo, *hi;
    const uint64_t *alpha;
    ScaleTables S;
    uint32_t inv2_m;
    // LEAF_COMBINE
    const uint32_t *cols;
    size_t stride;
    uint32_t n_cols;
    const uint32_t *weights_m;   // (weight mod p) in Montgomery form, on the device (fs_weights_kernel)
};
// Fri::commit (+ the query phase of Fri::prove with do_query) over a device codeword (fri.hip).
struct FriRequest {
    const smi_fri_cfg *cfg;
    const uint32_t *d_codeword;   // cfg->domain_length elements; with round0_src: the buffer the first tree's launch fills
    size_t len;
    bool do_query;
    bool reset_arena = true;    // false: the caller's own buffers of this prove live in the arena
    bool retain = false;        // true: the codewords and trees outlive the call (FriResult::run, hipMalloc); false: arena
    const LeafSrc *round0_src = nullptr;   // LEAF_COMBINE: the initial codeword is computed by the launch that hashes it
    const FsSeed *seed = nullptr;          // nullptr: a fresh FiatShamir
    // a few device bytes of the caller's (the column roots of a prove) that ride back with the single copy-back
    const void *ride_src = nullptr;
    size_t ride_bytes = 0;
    void *ride_dst = nullptr;              // host
    FriRequest(const smi_fri_cfg *c, const uint32_t *cw, size_t n, bool query) : cfg(c), d_codeword(cw), len(n), do_query(query) {}
};
struct FriResult {
    FriLayout lay;                  // rounds, last_n and where things are in `proof`
    std::vector<uint8_t> proof;     // serialized ProofStream: root r at 33 r + 1, the last codeword's u64s at off_last + 9
    std::vector<uint64_t> alphas;   // R - 1 unreduced challenges (R entries)
    std::vector<uint64_t> top;      // top-level indices (do_query)
    smi_fri_run *run = nullptr;     // retain
};
int fri_run(smi_ctx *ctx, const FriRequest &rq, FriResult *res);

// Fri::prove over the quartic extension (fri.hip): the plain loop row tree -> Fiat-Shamir round -> fold -> ... -> query ->
// emit over a codeword of four coordinate columns `stride` apart; everything stays on the device until one copy-back.
struct FriExtResult {
    std::vector<uint8_t> proof;
    std::vector<uint64_t> top;      // top-level indices
    uint64_t nonce = 0;             // the proof-of-work nonce (grind != SMI_GRIND_NONE)
};
// grind: the proof-of-work difficulty (include/stark_mi.h, "Grinding"), 0 .. SMI_GRIND_MAX_BITS, or SMI_GRIND_NONE: no
// nonce record and no absorb -- the stream of smi_dev_fri_prove_ext.  The verifier (verify.hip) takes the same argument.
#define SMI_GRIND_NONE (-1)
int fri_run_ext(smi_ctx *ctx, const smi_fri_cfg *cfg, const FsSeed *seed, const uint32_t *d_codeword, size_t len, size_t stride, bool reset_arena,
                FriExtResult *res, int grind = SMI_GRIND_NONE);
int grind_bits_check(smi_ctx *ctx, uint32_t bits);   // SMI_ERR_BAD_ARG above SMI_GRIND_MAX_BITS (fri.hip)
// the AIR proof over FRI at folding factor 4 compares the composition with the layer-0 coset record: refused (SMI_ERR_BAD_ARG)
// by prover and verifier when the FRI part has no fold
#define AIR_FOLD4_NO_LAYER "air fold4: FRI has no fold at this shape (F = 0), so there is no layer-0 coset to compare the composition with"
// extension FRI at folding factor 4 (fri.hip): the nonce is always searched, res->nonce always set
int fri_run_ext_fold4(smi_ctx *ctx, const smi_fri_cfg *cfg, const FsSeed *seed, const uint32_t *d_codeword, size_t len, size_t stride, bool reset_arena,
                      FriExtResult *res, uint32_t grind_bits);

// launches (defined in the .hip files; every function one .hip file defines and another calls is declared here, once --
// the MgSide ones in mgpu_core.h)
// hash.hip
int launch_leaf_hash(smi_ctx *ctx, const uint32_t *d_elems, size_t n, uint8_t *d_digests);
int launch_combine(smi_ctx *ctx, const uint8_t *d_in, size_t n_pairs, uint8_t *d_out);
int launch_hash_bytes(smi_ctx *ctx, const uint8_t *d_msg, size_t len, uint32_t *d_out);
int launch_hash_bytes_batch(smi_ctx *ctx, const uint8_t *d_msgs, size_t n, size_t len, uint32_t *d_out);
int launch_verify_paths(smi_ctx *ctx, const uint8_t *d_leaves, const uint64_t *d_idx, const uint8_t *d_paths, size_t k, uint32_t depth,
                        const uint8_t *d_root, uint8_t *d_ok);
int launch_merkle(smi_ctx *ctx, const uint32_t *d_elems, size_t n, uint8_t *d_nodes);
int launch_merkle_fs(smi_ctx *ctx, const uint32_t *d_elems, size_t n, uint8_t *d_nodes, uint32_t *fs_words, uint8_t *proof_slot,
                     uint64_t *alpha_out, bool *done);
int launch_merkle_src_fs(smi_ctx *ctx, const LeafSrc &src, size_t n, uint8_t *d_nodes, uint32_t *fs_words, uint8_t *proof_slot,
                         uint64_t *alpha_out, bool *done);
int launch_merkle_rows(smi_ctx *ctx, const uint32_t *d_cols, uint32_t n_cols, size_t col_stride, size_t n, uint8_t *d_nodes);
// zk.hip: q (four coordinate columns of N words) += r
int zk_mask_add_launch(smi_ctx *ctx, uint32_t *d_q, size_t q_stride, const uint32_t *d_r, size_t r_stride, size_t N);
int launch_merkle_cosets(smi_ctx *ctx, const uint32_t *d_cols, uint32_t n_cols, size_t col_stride, size_t n, uint8_t *d_nodes);
int launch_merkle_batch(smi_ctx *ctx, const uint32_t *d_elems, size_t n, uint8_t *d_nodes, uint32_t n_trees, size_t elem_stride,
                        size_t node_stride_bytes, uint32_t row_cols = 0, size_t row_stride = 0);
// fri.hip
int launch_fold_shard(smi_ctx *ctx, const uint32_t *d_lo, const uint32_t *d_hi, size_t count, size_t i0, size_t full_len,
                      const uint64_t *d_alpha, uint64_t offset, uint64_t omega, uint32_t *d_out);
// the x^-1 table of the fold out of a codeword of len elements on offset * <omega> (src/ff.rs:182: no division by zero)
int fri_fold_tables(smi_ctx *ctx, uint32_t offset, uint32_t omega, uint64_t len, ScaleTables *S);
int ext_field_check(smi_ctx *ctx);   // SMI_ERR_BAD_ARG unless X^4 - g is irreducible over the context's field (fri_core.h)
inline uint32_t fri_inv2_m(const smi_ctx *c) { return (uint32_t)(((uint64_t)h_inv(c, 2) << 32) % c->fs.F.p); }   // 2^-1, Montgomery form
int launch_fs_init(smi_ctx *ctx, void *fs, const FsSeed *seed);   // seed == nullptr: a fresh transcript
int launch_fs_round(smi_ctx *ctx, void *fs, const uint8_t *root, uint8_t *proof_slot, uint64_t *alpha_out, uint32_t phase);
int launch_fs_challenge(smi_ctx *ctx, const void *fs, uint64_t *out, uint32_t phase);
int launch_sample_indices(smi_ctx *ctx, const uint64_t *challenge, uint64_t size, uint64_t reduced_size, uint32_t number,
                          uint64_t *indices, uint64_t *reduced);
int launch_emit_codeword(smi_ctx *ctx, const uint32_t *cw, uint64_t len, uint8_t *dst);
// stark.hip
int launch_fs_weights(smi_ctx *ctx, const uint8_t *const *d_root_ptrs, uint32_t n, uint64_t *weights, uint8_t *roots_out);
// ntt.hip
int launch_geom_table(smi_ctx *ctx, const GeomSpec &s, uint32_t *d_out);
int launch_narrow(smi_ctx *ctx, const uint64_t *d_in, uint32_t *d_out, size_t n, int reduce);
int launch_widen(smi_ctx *ctx, const uint32_t *d_in, uint64_t *d_out, size_t n);
int dev_ntt(smi_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, uint32_t log_n, size_t n_in, uint32_t batch,
            size_t in_stride, size_t out_stride, int inverse, uint64_t offset, uint64_t post_scale);
int dev_lde2(smi_ctx *ctx, const uint32_t *d_coef, uint32_t *d_out, uint32_t log_n, uint32_t log_blowup, uint32_t batch,
             size_t coef_stride, size_t out_stride);
int dev_ntt_shard_first(smi_ctx *ctx, uint32_t *d_strip, uint32_t log_n, uint32_t log_g, uint32_t rank, int inverse, uint64_t offset);
int dev_ntt_shard_rest(smi_ctx *ctx, uint32_t *d_rows, uint32_t *d_out, uint32_t log_n, uint32_t log_g, int inverse);
// g = rb^-1 mod x^k by Newton iteration, rb[0] = 1 / g0 (poly.hip): e k words, f1 and f2 2^L >= 2k - 1 words each
int dev_series_inv(smi_ctx *ctx, const uint32_t *rb, size_t k, uint32_t g0, uint32_t *g, uint32_t *e, uint32_t *f1, uint32_t *f2);
int check_flag(smi_ctx *ctx);  // syncs; SMI_ERR_NON_CANONICAL if a narrow kernel saw a value >= p
// caller's (pageable) u64 buffers <-> device u32 residues; synchronous on return
int host_to_dev_u32(smi_ctx *ctx, const uint64_t *host, size_t n, uint32_t *d_out, int reduce);
int dev_u32_to_host(smi_ctx *ctx, const uint32_t *d_in, size_t n, uint64_t *host);
// air.hip: the periodic operands of an AIR (air_core.h) at the points idx -- out[q * 2Q + j] = pi_j(x_idx[q]),
// out[q * 2Q + Q + j] = pi_j(w x_idx[q]) -- from tables built on the device as the prover builds them; synchronises
struct AirHost;
int air_periodic_at(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, const std::vector<uint64_t> &idx, std::vector<uint32_t> *out);
// air.hip, for perm.hip: the validated tables of (cfg, air) bound to host memory; the blob to d_blob and the launch of the
// extension composition (binds H to d_blob); air_row_open_kernel on the context's stream; the periodic tables on the stream
struct smi_air;
int air_host_tables(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, AirHost *H, uint64_t *E);
int air_compose_ext_launch(smi_ctx *ctx, AirHost &H, uint32_t *d_blob, const uint32_t *d_lde, size_t stride, const uint64_t *d_weights, uint32_t *d_out,
                           size_t out_stride);
int launch_air_row_open(smi_ctx *ctx, const uint32_t *d_cols, size_t stride, uint32_t W, const uint8_t *d_nodes, uint32_t depth, const uint64_t *d_top,
                        uint32_t t, uint32_t R, uint64_t B, uint8_t *d_out);
// args.hip, for xargs.hip: the scan and propagation launches of a column build whose block launch has filled d_c and d_agg
// (SD: args_dev.h), and the flags the build leaves on the device
struct ArgsScanDev;
struct ArgsFlags {   // the totals (plain), the smallest key 16 row + 2 a + side
    uint32_t total[8][4];
    unsigned long long first;
    unsigned long long pad;
};
int args_scan_propagate_enqueue(smi_ctx *ctx, const ArgsScanDev &SD, uint64_t n, bool vec, uint32_t *d_c, size_t c_stride, uint32_t *d_agg, ArgsFlags *d_fl);
int air_periodic_tables(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, uint32_t *d_vals, uint32_t *d_tab);
// xargs.hip, for args.hip (a plain list runs these with its own checks in front), deep.hip and zkargs.hip: the entry checks;
// the column build's three launches over caller-owned temporary memory (xargs_columns_tmp_bytes bytes, 16-byte aligned;
// XD.pvals on the device), where the build leaves its flags in that memory, the verdicts of a finished build -- a zero
// denominator's sentence starts with `who` and calls a permutation's right side `perm_right` --, and the launch of the 2 A
// auxiliary quotients (H bound to the device blob, its periodic tables in place; d_w: the 8 A coordinates behind the main
// weights)
struct XArgsDev;
struct XSharedDev;   // the tuples of a list with a shared lookup; nullptr below: the list has none
int xargs_args(smi_ctx *ctx, const smi_air *air, const smi_air_xargs *xargs, uint32_t n_cols, uint32_t log_n);
size_t xargs_columns_tmp_bytes(uint32_t A, uint64_t n);
int xargs_columns_enqueue(smi_ctx *ctx, const XArgsDev &XD, const XSharedDev *SH, const uint32_t *d_trace, uint32_t log_n, uint32_t *d_c, size_t c_stride, uint8_t *d_tmp);
const ArgsFlags *xargs_columns_flags(const uint8_t *d_tmp, uint32_t A, uint64_t n);
int xargs_columns_verdict(smi_ctx *ctx, const XArgsDev &XD, const XSharedDev *SH, const ArgsFlags &fl, uint32_t *closes, const char *who = "xargs_columns",
                          const char *perm_right = "g_R");
int xargs_compose_enqueue(smi_ctx *ctx, const XArgsDev &XD, const XSharedDev *SH, const AirHost &H, uint32_t tau, const uint32_t *d_lde, size_t stride, const uint32_t *d_cl,
                          size_t c_stride, const uint64_t *d_w, uint32_t *d_out, size_t out_stride);
// xargs.hip, for args.hip: what the entry points of both lists run behind their checks -- the column build with its wait and
// verdicts, the main composition plus the auxiliary quotients, the prover.  air: the AIR whose periodic columns the operands
// may name, nullptr for a plain list; nm: the entry points' own words in the sentences these can fail with
struct ListNames {
    const char *columns, *perm_right;   // a zero denominator: "args_columns", "f_R" / "xargs_columns", "g_R"
    const char *prove;                  // out of memory: "air_prove_args" / "air_prove_xargs"
};
int xargs_columns_run(smi_ctx *ctx, const smi_air *air, const smi_air_xargs *xargs, const ListNames &nm, const uint32_t *d_trace_cols, uint32_t n_cols,
                      uint32_t log_n, const uint64_t *challenges, uint32_t *d_c, size_t c_stride, uint32_t *closes);
int xargs_compose_run(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, const smi_air *air, const smi_air_xargs *xargs, const uint32_t *d_lde, size_t stride,
                      const uint32_t *d_c_lde, size_t c_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out, size_t out_stride);
int xargs_prove_run(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, uint64_t E, const smi_air *air, const smi_air_xargs *xargs, const ListNames &nm,
                    const uint32_t *d_trace_cols, uint8_t *roots_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms,
                    uint32_t grind_bits, uint32_t *closes);
// perm.hip, for lookup.hip, args.hip and xargs.hip: the prover of every proof with two row trees, one over the extended trace
// and one over A auxiliary columns built under the challenges of the first root (4 A coordinate columns; the composition takes
// 2 A weights more).  The entry point has run its checks and its plan (H, E); the variant says how its columns are built,
// judged and composed.  DESIGN.md, "Where a new two-tree variant plugs in".
struct TwoTreeVariant {
    const char *name;               // the entry point, for the two out-of-memory sentences
    uint32_t A;                     // auxiliary columns
    size_t tmp_bytes;               // temporary device memory of the column build
    size_t flags_bytes;             // the build leaves its flags in the last flags_bytes of it (at most sizeof(ArgsFlags))
    // the tables under alpha, gamma = ch[0 .. 7] and the launches of the column build: d_c gets 4 A columns n apart.
    // d_pvals: the AIR's raw periodic values on the device (nullptr without periodic columns)
    std::function<int(const uint64_t *ch, const uint32_t *d_pvals, uint32_t *d_c, uint8_t *d_tmp)> columns;
    std::function<int(const void *flags)> settle;   // the flags on the host -> the caller's closes, or the failure
    // d_cw (the main composition, four columns N apart) += the 2 A auxiliary quotients under d_w; every stride is N
    std::function<int(const AirHost &H, const uint32_t *d_lde, const uint32_t *d_cl, const uint64_t *d_w, uint32_t *d_cw)> compose;
};
int two_tree_prove(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, uint64_t E, const uint32_t *d_trace_cols, const TwoTreeVariant &v, uint8_t *roots_out,
                   uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits);
// zkargs.hip, for deep.hip (the prover of "Zero-knowledge DEEP proofs with an argument list"): the tail step of the auxiliary
// columns (d_total: 4 A words for the closing values, d_rnd: 4 A (k_t - 1) random words) and the launch of the 3 A auxiliary
// quotients over the derived AIR's tables
int zk_args_tail_launch(smi_ctx *ctx, uint32_t *d_c, size_t c_stride, uint32_t log_n, uint32_t kt, uint32_t A, const uint32_t *d_rnd, uint32_t *d_total);
int zkx_compose_launch(smi_ctx *ctx, const XArgsDev &XD, const XSharedDev *SH, const AirHost &H, uint32_t tau, uint32_t log_n, uint32_t kt, const uint32_t *d_lde, size_t stride,
                       const uint32_t *d_cl, size_t c_stride, const uint64_t *d_w, uint32_t *d_out, size_t out_stride);
