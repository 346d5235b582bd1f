// fri.hip -- FRI fold kernel, on-device Fiat-Shamir / index sampling, query gather, and
// the host orchestration of Fri::commit / Fri::prove (reference src/fri.rs:57-311).
//
// The round loop of src/fri.rs:116-148 has a serial dependency root -> alpha -> fold
// (SURVEY H5).  Here the transcript state lives on the device: a single-lane kernel absorbs
// each root and draws alpha into device memory, the fold kernel reads alpha from there, so
// a whole prove is enqueued without one host round trip; the host synchronises once to
// copy the serialized proof back.
#include <assert.h>

#include "fri_core.h"
#include "hash_core.h"
#include "hash_hex.h"
#include "internal.h"

// ------------------------------------------------------------------------- fold
// out[i] = 2^-1 * ((1 + a/x_i) c[i] + (1 - a/x_i) c[i+h])            (src/fri.rs:70-88)
//        = 2^-1 (c[i] + c[i+h]) + (a * 2^-1 * x_i^-1) (c[i] - c[i+h]),  x_i = offset * omega^i
// x_i^-1 comes from the two-level table S = offset^-1 * omega^-i; alpha is read from device
// memory (unreduced u64, src/fiat_shamir.rs:23-24) and reduced here.  HBM-bound: 12 B in,
// 4 B out per output element.
__global__ __launch_bounds__(256) void fri_fold_kernel(const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                       uint32_t *__restrict__ out, uint32_t count, uint32_t i0,
                                                       const uint64_t *__restrict__ alpha_ptr, Fp F, ScaleTables S, uint32_t inv2_m) {
    const uint32_t ah_m = fold_alpha_half(*alpha_ptr, inv2_m, F);
    const uint32_t step = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += step)
        out[i] = fold_element(lo[i], hi[i], i0 + i, ah_m, inv2_m, S, F);
}

// ------------------------------------------------------------------------- Fiat-Shamir
// FiatShamir::{absorb,challenge} (src/fiat_shamir.rs:15-25).  Only whole 32-byte roots are
// ever absorbed (src/fri.rs:131), so the sponge state after k roots is carried in
// fs_state (16 words) and `challenge` = 8 more mixes on a copy: the same function of the
// whole transcript as re-hashing it, evaluated incrementally.
// A caller's transcript that is not whole 32-byte chunks leaves `phase` bytes pending (hash_core.h fs_seed); the phase
// rides in the state (FsSeed, transcript_core.h) so that the phase-aware kernels below read it with the words.

// the seed (the initial constants for a fresh transcript) arrives by value: it is computed on the host
// (ride_*: a few bytes of the caller's -- the column roots of a prove -- placed behind the proof, to come back with its copy)
__global__ void fs_init_kernel(FsSeed *fs, FsSeed seed, const uint8_t *ride_src = nullptr, uint8_t *ride_dst = nullptr, size_t ride_n = 0) {
    if (blockIdx.x) return;
    for (size_t i = threadIdx.x; i < ride_n; i += blockDim.x) ride_dst[i] = ride_src[i];
    if (threadIdx.x) return;
    for (int i = 0; i < 16; i++) fs->s[i] = seed.s[i];
    fs->phase = seed.phase;
}

// absorb the root at `root`, append it (tag 0 + 32 bytes, src/stream.rs:39-42) to the proof
// buffer, and if alpha_out != nullptr draw the challenge.
// (both over the first sixteen lanes, one state word each: hash_hex.h)
__global__ void fs_round_kernel(FsSeed *fs, const uint32_t *root, uint8_t *proof_slot, uint64_t *alpha_out) {
    if (threadIdx.x >= 16 || blockIdx.x) return;
    const hashx::Lane row = hashx::make_lane(threadIdx.x);
    const uint32_t j = threadIdx.x >> 2;
    hashx::fs_absorb_root(fs->s, hashx::message(root[j], root[4 + j], row), row, proof_slot, alpha_out);
}

// challenge without absorbing (src/fri.rs:272: the index-sampling seed)
__global__ void fs_challenge_kernel(const FsSeed *fs, uint64_t *alpha_out) {
    if (threadIdx.x >= 16 || blockIdx.x) return;
    const hashx::Lane row = hashx::make_lane(threadIdx.x);
    const uint64_t a = hashx::low_bytes_u64(hashx::fs_challenge(fs->s[threadIdx.x], row));
    if (threadIdx.x == 0) *alpha_out = a;
}

// The same two at a phase != 0 (hash_core.h fs_absorb_root_phase / fs_challenge_phase), one lane: the root straddles
// two chunks there, which the sixteen-lane form does not cover.  Run once per round on a few hundred bytes of state.
__global__ void fs_round_phase_kernel(FsSeed *fs, const uint32_t *root, uint8_t *proof_slot, uint64_t *alpha_out) {
    if (threadIdx.x || blockIdx.x) return;
    uint32_t m[8];
    for (int j = 0; j < 8; j++) m[j] = root[j];
    hashc::fs_absorb_root_phase(fs->s, m, fs->phase, proof_slot, alpha_out);
}
__global__ void fs_challenge_phase_kernel(const FsSeed *fs, uint64_t *alpha_out) {
    if (threadIdx.x || blockIdx.x) return;
    *alpha_out = hashc::fs_challenge_phase(fs->s, fs->phase);
}

// Fri::sample_indices (src/fri.rs:176-213) with seed = Hash::from_u64(challenge).0
// (src/fri.rs:272, src/hash.rs:37-39).  One wave: lane l hashes seed||counter for counter =
// 64*batch + l, then lane 0 accepts candidates in counter order exactly like the reference's
// sequential loop (distinct modulo reduced_size).  `number` <= reduced_size is checked on the host.
__global__ __launch_bounds__(64) void sample_indices_kernel(const uint64_t *challenge, uint64_t size, uint64_t reduced_size,
                                                            uint32_t number, uint64_t *indices, uint64_t *reduced) {
    __shared__ uint64_t cand[64], cand_r[64];
    __shared__ uint64_t s_red[256];   // accepted reduced indices, mirrored in LDS: the acceptance loop is O(number^2) look-ups
    __shared__ uint32_t s_cnt;
    const uint32_t lane = threadIdx.x;
    // seed = hash of the 8 LE bytes of the (unreduced) challenge; every lane computes it (uniform)
    const uint64_t ch = *challenge;
    hashc::State st;
    hashc::init(st);
#pragma unroll
    for (int i = 0; i < 8; i++) hashc::absorb_byte(st, i, (uint32_t)(ch >> (8 * i)) & 0xFFu);
    hashc::mix(st);
    for (int k = 0; k < 8; k++) hashc::mix(st);
    uint32_t seed[8];
    hashc::to_words(st, seed);
    hashc::State base;   // state after the first chunk (= seed) of every seed||counter message
    hashc::init(base);
    hashc::absorb_chunk32(base, seed);
    if (lane == 0) s_cnt = 0;
    uint64_t held[4] = {0, 0, 0, 0};
    __syncthreads();
    for (uint32_t batch = 0; batch < (1u << 20); batch++) {   // bounded: ends as soon as `number` are accepted
        const uint32_t counter = batch * 64u + lane;
        hashc::State s2 = base;
#pragma unroll
        for (int i = 0; i < 4; i++) hashc::absorb_byte(s2, i, (counter >> (8 * i)) & 0xFFu);
        hashc::mix(s2);
        for (int k = 0; k < 8; k++) hashc::mix(s2);
        uint32_t d[8];
        hashc::to_words(s2, d);
        // sample_index (src/fri.rs:168-174): u128 shift-xor over 32 bytes, truncated to usize
        // = the last 8 digest bytes read big-endian
        uint64_t acc = 0;
#pragma unroll
        for (int i = 24; i < 32; i++) acc = (acc << 8) | ((d[i >> 2] >> (8 * (i & 3))) & 0xFFu);
        // both moduli are powers of two on every FRI path (lengths of codewords): a mask instead of
        // a 64-bit division; every lane reduces its own candidate, lane 0 only compares
        const uint64_t index_l = (size & (size - 1)) ? acc % size : acc & (size - 1);
        cand[lane] = index_l;
        cand_r[lane] = (reduced_size & (reduced_size - 1)) ? index_l % reduced_size : index_l & (reduced_size - 1);
        __syncthreads();
        if (number <= 256) {
            // acceptance in candidate order, the look-up spread over the wave: lane l keeps the accepted
            // reduced indices l, l+64, l+128, l+192 in registers and a ballot answers "seen before?"
            uint32_t cnt = s_cnt;   // wave-uniform
            for (uint32_t k = 0; k < 64 && cnt < number; k++) {
                const uint64_t index = cand[k], ri = cand_r[k];
                bool hit = false;
#pragma unroll
                for (uint32_t m = 0; m < 4; m++) hit |= lane + 64u * m < cnt && held[m] == ri;
                if (__ballot(hit) == 0) {
#pragma unroll
                    for (uint32_t m = 0; m < 4; m++)
                        if ((cnt >> 6) == m && (cnt & 63u) == lane) held[m] = ri;
                    if (lane == 0) {
                        indices[cnt] = index;
                        reduced[cnt] = ri;
                    }
                    cnt++;
                }
            }
            __syncthreads();
            if (lane == 0) s_cnt = cnt;
        } else if (lane == 0) {
            uint32_t cnt = s_cnt;
            for (uint32_t k = 0; k < 64 && cnt < number; k++) {
                const uint64_t index = cand[k], ri = cand_r[k];
                bool seen = false;
                for (uint32_t j = 0; j < cnt; j++) seen |= (j < 256 ? s_red[j] : reduced[j]) == ri;
                if (!seen) {
                    indices[cnt] = index;
                    reduced[cnt] = ri;
                    if (cnt < 256) s_red[cnt] = ri;
                    cnt++;
                }
            }
            s_cnt = cnt;
        }
        __syncthreads();
        if (s_cnt >= number) break;
    }
}

// ------------------------------------------------------------------------- query gather
// Fri::query (src/fri.rs:215-248) for every layer, written straight into the serialized
// ProofStream layout (src/stream.rs:35-64).  One workgroup per (layer, test).
struct LayerInfo {
    const uint32_t *cw, *cw_next;
    const uint8_t *nodes, *nodes_next;
    uint64_t len;           // of cw
    uint64_t off_triples;   // byte offset of this layer's first FieldElements triple
    uint64_t off_paths;     // byte offset of this layer's first MerklePath
    uint32_t depth, depth_next;
};

__device__ void put_u64(uint8_t *p, uint64_t v) {
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
// MerkleTree::open (src/merkle.rs:67-80) serialized as tag 3, u64 count, 32 B digests
__device__ void write_path(uint8_t *dst, const uint8_t *nodes, uint64_t n, uint32_t depth, uint64_t index, uint32_t lane) {
    if (lane == 0) {
        dst[0] = 3;
        put_u64(dst + 1, depth);
    }
    uint64_t idx = index, lvl_off = 0, len = n;
    for (uint32_t l = 0; l < depth; l++) {
        const uint64_t sib = idx ^ 1;
        if (lane < 32) dst[9 + 32 * l + lane] = nodes[(lvl_off + sib) * 32 + lane];
        idx >>= 1;
        lvl_off += len;
        len >>= 1;
    }
}
// The layer table travels as a kernel argument while it fits (SMI_QUERY_TAB_MAX layers: codewords of up to 2^40
// elements): a host-to-device copy between the index sampling and this launch would sit on the critical path of
// the prove with the runtime's gaps around it (profiles/r03_b_prove_timeline.txt).
#define SMI_QUERY_TAB_MAX 40
struct LayerTable {
    LayerInfo l[SMI_QUERY_TAB_MAX];
};
__device__ __forceinline__ void query_one(const LayerInfo &L, const uint64_t *top, uint8_t *proof);
__global__ void query_kernel(const LayerInfo *layers, const uint64_t *top, uint32_t t, uint8_t *proof) {
    const LayerInfo L = layers[blockIdx.y];
    query_one(L, top, proof);
}
__global__ void query_tab_kernel(const LayerTable tab, const uint64_t *top, uint32_t t, uint8_t *proof) {
    const LayerInfo L = tab.l[blockIdx.y];
    query_one(L, top, proof);
}
__device__ __forceinline__ void query_one(const LayerInfo &L, const uint64_t *top, uint8_t *proof) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint64_t half = L.len / 2;
    const uint64_t c = top[s] % half;   // indices folded layer by layer: (x % a) % b == x % b for b | a
    if (lane == 0) {
        uint8_t *tr = proof + L.off_triples + (uint64_t)s * 33;
        tr[0] = 2;
        put_u64(tr + 1, 3);
        put_u64(tr + 9, L.cw[c]);
        put_u64(tr + 17, L.cw[c + half]);
        put_u64(tr + 25, L.cw_next[c]);
    }
    const uint64_t pa = 9 + 32ull * L.depth, pc = 9 + 32ull * L.depth_next;
    uint8_t *pp = proof + L.off_paths + (uint64_t)s * (2 * pa + pc);
    write_path(pp, L.nodes, L.len, L.depth, c, lane);
    write_path(pp + pa, L.nodes, L.len, L.depth, c + half, lane);
    write_path(pp + 2 * pa, L.nodes_next, half, L.depth_next, c, lane);
}

// last codeword in the clear: tag 2, u64 len, len x u64 (src/fri.rs:151, src/stream.rs:48-53)
__global__ void emit_codeword_kernel(const uint32_t *cw, uint64_t len, uint8_t *dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        dst[0] = 2;
        put_u64(dst + 1, len);
    }
    if (i < len) put_u64(dst + 9 + 8 * i, cw[i]);
}

// launchers for the multi-GPU round loop (mgpu.hip), which sequences the same kernels
// (seed == nullptr: a fresh transcript; phase: the seed's, which the caller keeps on the host to pick the kernels)
int launch_fs_init(smi_ctx *ctx, void *fs, const FsSeed *seed) {
    fs_init_kernel<<<1, 64, 0, ctx->stream>>>((FsSeed *)fs, seed ? *seed : fresh_seed());
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
int launch_fs_round(smi_ctx *ctx, void *fs, const uint8_t *root, uint8_t *proof_slot, uint64_t *alpha_out, uint32_t phase) {
    if (phase) fs_round_phase_kernel<<<1, 64, 0, ctx->stream>>>((FsSeed *)fs, (const uint32_t *)root, proof_slot, alpha_out);
    else fs_round_kernel<<<1, 64, 0, ctx->stream>>>((FsSeed *)fs, (const uint32_t *)root, proof_slot, alpha_out);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
int launch_fs_challenge(smi_ctx *ctx, const void *fs, uint64_t *out, uint32_t phase) {
    if (phase) fs_challenge_phase_kernel<<<1, 64, 0, ctx->stream>>>((const FsSeed *)fs, out);
    else fs_challenge_kernel<<<1, 64, 0, ctx->stream>>>((const FsSeed *)fs, out);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
int launch_sample_indices(smi_ctx *ctx, const uint64_t *challenge, uint64_t size, uint64_t reduced_size, uint32_t number,
                          uint64_t *indices, uint64_t *reduced) {
    sample_indices_kernel<<<1, 64, 0, ctx->stream>>>(challenge, size, reduced_size, number, indices, reduced);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
int launch_emit_codeword(smi_ctx *ctx, const uint32_t *cw, uint64_t len, uint8_t *dst) {
    emit_codeword_kernel<<<(uint32_t)((len + 255) / 256), 256, 0, ctx->stream>>>(cw, len, dst);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

// ------------------------------------------------------------------------- host side
int smi_fri_num_rounds(const smi_fri_cfg *cfg, uint64_t *rounds) {
    if (!cfg || !rounds) return SMI_ERR_BAD_ARG;
    *rounds = fri_layout(*cfg, false).R;   // src/fri.rs:93-103
    return SMI_OK;
}

int smi_fri_check(const smi_ctx *ctx, const smi_fri_cfg *cfg) {
    if (!ctx || !cfg) return SMI_ERR_BAD_ARG;
    if (!is_pow2(cfg->domain_length)) return SMI_ERR_DOMAIN_NOT_POW2;      // src/fri.rs:37-40
    if (!is_pow2(cfg->expansion_factor)) return SMI_ERR_EXPANSION_NOT_POW2;  // src/fri.rs:41-44
    if (cfg->expansion_factor < 4) return SMI_ERR_EXPANSION_TOO_SMALL;       // src/fri.rs:45
    return SMI_OK;
}

int smi_fri_fold4_layout(const smi_fri_cfg *cfg, uint64_t *folds, uint64_t *last_len, size_t *proof_len) {
    if (!cfg || !folds || !last_len || !proof_len) return SMI_ERR_BAD_ARG;
    if (!is_pow2(cfg->domain_length)) return SMI_ERR_DOMAIN_NOT_POW2;
    if (!is_pow2(cfg->expansion_factor)) return SMI_ERR_EXPANSION_NOT_POW2;
    if (cfg->expansion_factor < 4) return SMI_ERR_EXPANSION_TOO_SMALL;
    const FriFold4Layout l = fri_layout_fold4(*cfg);
    if (l.R2 == 0) return SMI_ERR_NO_ROUNDS;
    *folds = l.F;
    *last_len = l.last_n;
    *proof_len = l.proof_len;
    return SMI_OK;
}

// Every device buffer of a run is handed to it at the moment it is allocated: smi_fri_run_free is the only place that frees.
struct smi_fri_run {
    smi_ctx *ctx;
    std::vector<uint32_t *> codewords;  // device, lengths N, N/2, ...
    std::vector<uint8_t *> trees;       // device nodes per codeword
    std::vector<uint64_t> lens;
    void *d_misc;                       // fs state, alphas, indices, layer table
    uint8_t *d_proof;
    bool owns_first;                    // codewords[0] allocated by us (vs caller's buffer)
    bool arena;                         // buffers live in the context arena (not retained past the call)
};
static void *run_alloc(smi_fri_run *run, size_t bytes) {
    if (run->arena) return arena_alloc(run->ctx, bytes);
    void *q = nullptr;
    if (hipMalloc(&q, bytes ? bytes : 4) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return q;
}
static uint32_t *run_codeword(smi_fri_run *run, uint64_t len) {
    uint32_t *cw = (uint32_t *)run_alloc(run, len * 4);
    if (cw) {
        run->codewords.push_back(cw);
        run->lens.push_back(len);
    }
    return cw;
}
static uint8_t *run_tree(smi_fri_run *run, uint64_t len) {
    uint8_t *nodes = (uint8_t *)run_alloc(run, (2 * len - 1) * 32);
    if (nodes) run->trees.push_back(nodes);
    return nodes;
}

void smi_fri_run_free(smi_fri_run *run) {
    if (!run) return;
    DeviceGuard dg__(run->ctx);
    if (run->arena) {  // arena memory is recycled by the next arena_reset
        if (run->owns_first && !run->codewords.empty()) {
            (void)hipStreamSynchronize(run->ctx->stream);
            (void)hipFree(run->codewords[0]);
        }
        delete run;
        return;
    }
    (void)hipStreamSynchronize(run->ctx->stream);
    for (size_t i = 0; i < run->codewords.size(); i++)
        if (i > 0 || run->owns_first) (void)hipFree(run->codewords[i]);
    for (uint8_t *t : run->trees) (void)hipFree(t);
    (void)hipFree(run->d_misc);
    (void)hipFree(run->d_proof);
    delete run;
}

int fri_fold_tables(smi_ctx *ctx, uint32_t offset, uint32_t omega, uint64_t len, ScaleTables *S) {
    if (len < 2 || !is_pow2(len)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fold: codeword length must be a power of two >= 2");
    if (offset == 0 || omega == 0) return smi_fail(ctx, SMI_ERR_DIV_BY_ZERO, "no division by zero");  // src/ff.rs:182
    return ctx_scale_tables(ctx, h_inv(ctx, offset), h_inv(ctx, omega), ilog2(len / 2), S);
}
static int launch_fold_tables(smi_ctx *ctx, const uint32_t *d_lo, const uint32_t *d_hi, size_t count, size_t i0, const uint64_t *d_alpha,
                              const ScaleTables &S, uint32_t inv2_m, uint32_t *d_out) {
    uint32_t grid = (uint32_t)((count + 255) / 256);
    if (grid > 2048) grid = 2048;
    ProfScope ps(ctx, "fri_fold_kernel", 12.0 * (double)count);  // read 2 x 4 B, write 4 B per output
    fri_fold_kernel<<<grid, 256, 0, ctx->stream>>>(d_lo, d_hi, d_out, (uint32_t)count, (uint32_t)i0, d_alpha, ctx->fs.F, S, inv2_m);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
// Folds `count` outputs starting at global index i0 of a codeword of length full_len:
// out[k] = fold(lo[k], hi[k]) where lo[k] = c[i0+k], hi[k] = c[i0+k+full_len/2].
int launch_fold_shard(smi_ctx *ctx, const uint32_t *d_lo, const uint32_t *d_hi, size_t count, size_t i0, size_t full_len,
                      const uint64_t *d_alpha, uint64_t offset, uint64_t omega, uint32_t *d_out) {
    const uint32_t p = ctx->fs.F.p;
    if (full_len < 2 || !is_pow2(full_len)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fold: codeword length must be a power of two >= 2");
    if (i0 + count > full_len / 2) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fold: shard outside the folded codeword");
    if (offset >= p || omega >= p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "fold: offset/omega must be < p");
    if (offset == 0 || omega == 0) return smi_fail(ctx, SMI_ERR_DIV_BY_ZERO, "no division by zero");  // (also for an empty shard)
    if (!count) return SMI_OK;
    ScaleScope pin__(ctx);
    ScaleTables S;
    SMI_TRY(fri_fold_tables(ctx, (uint32_t)offset, (uint32_t)omega, full_len, &S));
    return launch_fold_tables(ctx, d_lo, d_hi, count, i0, d_alpha, S, fri_inv2_m(ctx), d_out);
}
int smi_dev_fri_fold_shard(smi_ctx *ctx, const uint32_t *d_lo, const uint32_t *d_hi, size_t count, size_t index0, size_t full_len,
                           const uint64_t *d_alpha, uint64_t offset, uint64_t omega, uint32_t *d_out) {
    if (!ctx || !d_lo || !d_hi || !d_alpha || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return launch_fold_shard(ctx, d_lo, d_hi, count, index0, full_len, d_alpha, offset, omega, d_out);
}

// ------------------------------------------------------------------------- fold over the quartic extension
// The codeword is four coordinate columns `stride` apart (include/stark_mi.h, "Quartic extension"); element i of the
// next one is fold_element_ext (fri_core.h) of elements i and i + half.  8 words in, 4 out per output element: 48 B.
// VEC: a lane takes four consecutive elements, every access 16 bytes (all bases 16-byte aligned, strides and half
// multiples of 4); otherwise one element per lane, 4-byte accesses.  alpha: four unreduced u64 in device memory.
template <bool VEC>
__global__ __launch_bounds__(256) void fri_fold_ext_kernel(const uint32_t *__restrict__ in, size_t stride, uint32_t half,
                                                           const uint64_t *__restrict__ alpha_ptr, uint32_t g_m, Fp F, ScaleTables S,
                                                           uint32_t inv2_m, uint32_t *__restrict__ out, size_t out_stride) {
    const uint64_t a[4] = {alpha_ptr[0], alpha_ptr[1], alpha_ptr[2], alpha_ptr[3]};
    const ExtMul alpha = fold_ext_alpha(a, g_m, F);
    const uint32_t step = gridDim.x * blockDim.x;
    if constexpr (VEC) {
        for (uint32_t i = 4 * (blockIdx.x * blockDim.x + threadIdx.x); i < half; i += 4 * step) {
            uint32_t lo[4][4], hi[4][4], res[4][4];   // [coordinate][element]
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint4 l = *(const uint4 *)(in + e * stride + i), h = *(const uint4 *)(in + e * stride + half + i);
                lo[e][0] = l.x; lo[e][1] = l.y; lo[e][2] = l.z; lo[e][3] = l.w;
                hi[e][0] = h.x; hi[e][1] = h.y; hi[e][2] = h.z; hi[e][3] = h.w;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t l[4] = {lo[0][j], lo[1][j], lo[2][j], lo[3][j]}, h[4] = {hi[0][j], hi[1][j], hi[2][j], hi[3][j]};
                uint32_t o[4];
                fold_element_ext(l, h, i + j, alpha, inv2_m, S, F, o);
#pragma unroll
                for (int e = 0; e < 4; e++) res[e][j] = o[e];
            }
#pragma unroll
            for (int e = 0; e < 4; e++) *(uint4 *)(out + e * out_stride + i) = make_uint4(res[e][0], res[e][1], res[e][2], res[e][3]);
        }
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < half; i += step) {
            uint32_t l[4], h[4], o[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                l[e] = in[e * stride + i];
                h[e] = in[e * stride + half + i];
            }
            fold_element_ext(l, h, i, alpha, inv2_m, S, F, o);
#pragma unroll
            for (int e = 0; e < 4; e++) out[e * out_stride + i] = o[e];
        }
    }
}

// the context's (p, g) must make X^4 - g irreducible (fri_core.h ext_field_ok)
int ext_field_check(smi_ctx *ctx) {
    const char *why = nullptr;
    if (!ext_field_ok(ctx->fs.F.p, ctx->fs.g, &why)) return smi_fail(ctx, SMI_ERR_BAD_ARG, why);
    return SMI_OK;
}

static int launch_fold_ext(smi_ctx *ctx, const uint32_t *d_in, size_t len, size_t stride, const uint64_t *d_alpha, uint64_t offset, uint64_t omega,
                           uint32_t *d_out, size_t out_stride) {
    const uint32_t p = ctx->fs.F.p;
    if (len < 2 || !is_pow2(len) || len > ((size_t)1 << 27)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fold_ext: codeword length must be a power of two in 2 .. 2^27");
    const size_t half = len / 2;
    if (stride < len || out_stride < half) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fold_ext: stride < len or out_stride < len / 2");
    if (offset >= p || omega >= p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "fold: offset/omega must be < p");
    ScaleScope pin__(ctx);
    ScaleTables S;
    SMI_TRY(fri_fold_tables(ctx, (uint32_t)offset, (uint32_t)omega, len, &S));   // (refuses a zero offset / omega)
    const uint32_t g_m = (uint32_t)(((uint64_t)ctx->fs.g << 32) % p);
    const bool vec = !(half & 3) && !(stride & 3) && !(out_stride & 3) && !(((uintptr_t)d_in | (uintptr_t)d_out) & 15u);
    const size_t lanes = vec ? half / 4 : half;
    uint32_t grid = (uint32_t)((lanes + 255) / 256);
    if (grid > 2048) grid = 2048;
    ProfScope ps(ctx, "fri_fold_ext_kernel", 48.0 * (double)half);   // read 2 x 16 B, write 16 B per output element
    if (vec) fri_fold_ext_kernel<true><<<grid, 256, 0, ctx->stream>>>(d_in, stride, (uint32_t)half, d_alpha, g_m, ctx->fs.F, S, fri_inv2_m(ctx), d_out, out_stride);
    else fri_fold_ext_kernel<false><<<grid, 256, 0, ctx->stream>>>(d_in, stride, (uint32_t)half, d_alpha, g_m, ctx->fs.F, S, fri_inv2_m(ctx), d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
int smi_dev_fri_fold_ext(smi_ctx *ctx, const uint32_t *d_in, size_t len, size_t stride, const uint64_t *d_alpha, uint64_t offset, uint64_t omega,
                         uint32_t *d_out, size_t out_stride) {
    if (!ctx || !d_in || !d_alpha || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(ext_field_check(ctx));
    return launch_fold_ext(ctx, d_in, len, stride, d_alpha, offset, omega, d_out, out_stride);
}

// ------------------------------------------------------------------------- fold by 4 over the quartic extension
// Element i of the output (i < q = len / 4) is fold4_element_ext (fri_core.h) of elements i, i + q, i + 2 q, i + 3 q: the
// two folds fri_fold_ext_kernel makes in two launches, in registers.  16 words in, 4 out per output element: 80 B, against
// 96 + 48 for the pair.  VEC: a lane takes four consecutive outputs, every access 16 bytes (all bases 16-byte aligned;
// strides and q multiples of 4); otherwise one output per lane, 4-byte accesses.  The largest index read is
// 3 stride + 3 q + i < 4 stride, the largest written 3 out_stride + i < 4 out_stride.
template <bool VEC>
__global__ __launch_bounds__(256) void fri_fold4_ext_kernel(const uint32_t *__restrict__ in, size_t stride, uint32_t q,
                                                            const uint64_t *__restrict__ alpha_ptr, uint32_t g_m, Fp F, ScaleTables S,
                                                            uint32_t inv2_m, uint32_t iota_inv_m, uint32_t *__restrict__ out, size_t out_stride) {
    const uint64_t a[4] = {alpha_ptr[0], alpha_ptr[1], alpha_ptr[2], alpha_ptr[3]};
    const Fold4Alpha A = fold4_ext_alpha(a, g_m, F);
    const uint32_t step = gridDim.x * blockDim.x;
    if constexpr (VEC) {
        for (uint32_t i = 4 * (blockIdx.x * blockDim.x + threadIdx.x); i < q; i += 4 * step) {
            uint32_t v[4][4][4], res[4][4];   // v[coset slot][coordinate][element], res[coordinate][element]
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const uint4 w = *(const uint4 *)(in + e * stride + (size_t)j * q + i);
                    v[j][e][0] = w.x; v[j][e][1] = w.y; v[j][e][2] = w.z; v[j][e][3] = w.w;
                }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t c[4][4], o[4];
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int e = 0; e < 4; e++) c[j][e] = v[j][e][k];
                fold4_element_ext(c, i + k, A, inv2_m, iota_inv_m, S, F, o);
#pragma unroll
                for (int e = 0; e < 4; e++) res[e][k] = o[e];
            }
#pragma unroll
            for (int e = 0; e < 4; e++) *(uint4 *)(out + e * out_stride + i) = make_uint4(res[e][0], res[e][1], res[e][2], res[e][3]);
        }
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < q; i += step) {
            uint32_t c[4][4], o[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int e = 0; e < 4; e++) c[j][e] = in[e * stride + (size_t)j * q + i];
            fold4_element_ext(c, i, A, inv2_m, iota_inv_m, S, F, o);
#pragma unroll
            for (int e = 0; e < 4; e++) out[e * out_stride + i] = o[e];
        }
    }
}

// The grid is capped at 2048 workgroups of 256 lanes as launch_fold_ext's is: with four outputs a lane the grid-stride loop
// makes a second trip from q = 2^22 on, that is from len = 2^24.
static int launch_fold4_ext(smi_ctx *ctx, const uint32_t *d_in, size_t len, size_t stride, const uint64_t *d_alpha, uint64_t offset, uint64_t omega,
                            uint32_t *d_out, size_t out_stride) {
    const uint32_t p = ctx->fs.F.p;
    if (len < 4 || !is_pow2(len) || len > ((size_t)1 << 27)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fold4_ext: codeword length must be a power of two in 4 .. 2^27");
    const size_t q = len / 4;
    if (stride < len || out_stride < q) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fold4_ext: stride < len or out_stride < len / 4");
    if (offset >= p || omega >= p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "fold: offset/omega must be < p");
    ScaleScope pin__(ctx);
    ScaleTables S;
    SMI_TRY(fri_fold_tables(ctx, (uint32_t)offset, (uint32_t)omega, len / 2, &S));   // q entries; refuses a zero offset / omega
    const uint32_t g_m = (uint32_t)(((uint64_t)ctx->fs.g << 32) % p);
    const uint32_t iota_inv = host_powmod(h_inv(ctx, (uint32_t)omega), q, p), iota_inv_m = (uint32_t)(((uint64_t)iota_inv << 32) % p);
    const bool vec = !(q & 3) && !(stride & 3) && !(out_stride & 3) && !(((uintptr_t)d_in | (uintptr_t)d_out) & 15u);
    const size_t lanes = vec ? q / 4 : q;
    uint32_t grid = (uint32_t)((lanes + 255) / 256);
    if (grid > 2048) grid = 2048;
    ProfScope ps(ctx, "fri_fold4_ext_kernel", 80.0 * (double)q);   // read 4 x 16 B, write 16 B per output element
    if (vec) fri_fold4_ext_kernel<true><<<grid, 256, 0, ctx->stream>>>(d_in, stride, (uint32_t)q, d_alpha, g_m, ctx->fs.F, S, fri_inv2_m(ctx), iota_inv_m, d_out, out_stride);
    else fri_fold4_ext_kernel<false><<<grid, 256, 0, ctx->stream>>>(d_in, stride, (uint32_t)q, d_alpha, g_m, ctx->fs.F, S, fri_inv2_m(ctx), iota_inv_m, d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
int smi_dev_fri_fold4_ext(smi_ctx *ctx, const uint32_t *d_in, size_t len, size_t stride, const uint64_t *d_alpha, uint64_t offset, uint64_t omega,
                          uint32_t *d_out, size_t out_stride) {
    if (!ctx || !d_in || !d_alpha || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(ext_field_check(ctx));
    return launch_fold4_ext(ctx, d_in, len, stride, d_alpha, offset, omega, d_out, out_stride);
}

// F_q on the host, no context (smi_air_plan's kind): plain canonical coordinates in and out
static int ext_args(uint64_t p, uint64_t g, const uint64_t *a, const uint64_t *b) {
    if (!ext_field_ok(p, g, nullptr) || !is_prime_u32((uint32_t)p)) return SMI_ERR_BAD_ARG;
    for (int e = 0; e < 4; e++)
        if (a[e] >= p || (b && b[e] >= p)) return SMI_ERR_NON_CANONICAL;
    return SMI_OK;
}
int smi_ext_mul(uint64_t p, uint64_t g, const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
    if (!a || !b || !out) return SMI_ERR_BAD_ARG;
    SMI_TRY(ext_args(p, g, a, b));
    const uint32_t x[4] = {(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]}, y[4] = {(uint32_t)b[0], (uint32_t)b[1], (uint32_t)b[2], (uint32_t)b[3]};
    uint32_t r[4];
    ext_mul_host((uint32_t)p, (uint32_t)g, x, y, r);
    for (int e = 0; e < 4; e++) out[e] = r[e];
    return SMI_OK;
}
int smi_ext_inv(uint64_t p, uint64_t g, const uint64_t a[4], uint64_t out[4]) {
    if (!a || !out) return SMI_ERR_BAD_ARG;
    SMI_TRY(ext_args(p, g, a, nullptr));
    const uint32_t x[4] = {(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]};
    uint32_t r[4];
    if (!ext_inv_host((uint32_t)p, (uint32_t)g, x, r)) return SMI_ERR_NO_INVERSE;   // src/ff.rs:171
    for (int e = 0; e < 4; e++) out[e] = r[e];
    return SMI_OK;
}

// Codewords of at most this many elements finish in the fused tail launch (hash.hip, fri_tail_kernel).
// Measured on MI355X (2^25-point prove): the FRI stage is 4.44..4.69 ms with the tail
// off, from 512, from 1024 or from 2048 elements alike -- the differences are inside the run-to-run
// spread of +-0.1 ms, because the tail's cost is the serial chain tree -> alpha -> fold, not launch
// overhead.  Default: 512, the size the per-round path hands to a single workgroup anyway (above it
// the per-round path spreads a tree's 64-leaf chunks over several CUs).  SMI_FRI_TAIL=<len> overrides
// (0: never).
uint64_t fri_tail_len() {
    static const uint64_t tail_len = [] {
        const char *e = getenv("SMI_FRI_TAIL");
        const uint64_t v = e ? (uint64_t)atoll(e) : 512;
        return v > SMI_FRI_TAIL_MAX_LEN ? (uint64_t)SMI_FRI_TAIL_MAX_LEN : v;
    }();
    return tail_len;
}

// What the three parts of fri_run share.  Device block `misc`: fs state | seed challenge | reduced indices | layer table;
// the challenges, the sampled indices and the caller's ride-along bytes live behind the proof in ONE device buffer, so
// that everything the host needs comes back in a single device-to-host copy: four copies cost 17 + 5 + 4 + 4 us of blit
// kernels and 86 us of runtime gaps between them at the end of every prove (profiles/r03_b_prove_timeline.txt).
struct FriExec {
    smi_ctx *ctx;
    const FriRequest *rq;
    smi_fri_run *run;
    FriLayout lay;
    FriRoundPlan plan;
    uint32_t phase;
    size_t off_al, off_top, off_ride, back_len;   // in run->d_proof
    FsSeed *d_fs;
    uint64_t *d_alphas, *d_seed_ch, *d_top, *d_reduced;
    LayerInfo *d_layers;
};

// part 1: validate, lay out, allocate, start the transcript
static int fri_setup(FriExec &x) {
    smi_ctx *ctx = x.ctx;
    const FriRequest &rq = *x.rq;
    SMI_TRY(smi_fri_check(ctx, rq.cfg));
    if (rq.cfg->domain_length != rq.len) return smi_fail(ctx, SMI_ERR_CODEWORD_LEN, "initial codeword length does not match domain length");
    const uint32_t p = ctx->fs.F.p;
    if (rq.cfg->omega >= p || rq.cfg->offset >= p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "omega/offset must be < p");
    x.lay = fri_layout(*rq.cfg, rq.do_query);
    const uint64_t R = x.lay.R, t = rq.cfg->num_colinearity_tests;
    if (R == 0) return smi_fail(ctx, SMI_ERR_NO_ROUNDS, "num_rounds() == 0: the reference's verify rejects such a proof");
    if (rq.do_query) {  // asserts of src/fri.rs:183-192
        if (t > 2 * x.lay.last_n) return smi_fail(ctx, SMI_ERR_SAMPLE_ENTROPY, "not enough entropy in indices wrt last codeword");
        if (t > x.lay.last_n) return smi_fail(ctx, SMI_ERR_SAMPLE_TOO_MANY, "cannot sample more indices than available in last codeword");
    }
    const FsSeed fs0 = rq.seed ? *rq.seed : fresh_seed();
    x.phase = fs0.phase;
    const int round0 = rq.round0_src ? FRI_R0_COMBINE : (((uintptr_t)rq.d_codeword & 15u) ? FRI_R0_UNALIGNED : FRI_R0_ALIGNED16);
    x.plan = fri_round_plan(rq.len, R, x.phase, fri_tail_len(), round0, merkle_knobs_env());
    if (!x.plan.ok) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fri: the initial codeword is too short for a computed leaf source");

    smi_fri_run *run = x.run = new smi_fri_run{ctx, {}, {}, {}, nullptr, nullptr, false, !rq.retain};   // not retained: the arena
    if (run->arena && rq.reset_arena) (void)arena_reset(ctx);
    run->codewords.push_back(const_cast<uint32_t *>(rq.d_codeword));
    run->lens.push_back(rq.len);

    const size_t m_seed_ch = (sizeof(FsSeed) + 63) & ~(size_t)63, m_reduced = m_seed_ch + 8;
    const size_t m_layers = (m_reduced + 8 * (t + 1) + 63) & ~(size_t)63;
    if (!(run->d_misc = run_alloc(run, m_layers + sizeof(LayerInfo) * (R + 1)))) return smi_fail(ctx, SMI_ERR_OOM, "alloc misc");
    x.off_al = (x.lay.proof_len + 7) & ~(size_t)7;
    x.off_top = x.off_al + 8 * R;
    x.off_ride = x.off_top + 8 * (t + 1);
    x.back_len = x.off_ride + (rq.ride_src ? rq.ride_bytes : 0);
    if (!(run->d_proof = (uint8_t *)run_alloc(run, x.back_len))) return smi_fail(ctx, SMI_ERR_OOM, "alloc proof");
    uint8_t *misc = (uint8_t *)run->d_misc;
    x.d_fs = (FsSeed *)misc;
    x.d_seed_ch = (uint64_t *)(misc + m_seed_ch);
    x.d_reduced = (uint64_t *)(misc + m_reduced);
    x.d_layers = (LayerInfo *)(misc + m_layers);
    x.d_alphas = (uint64_t *)(run->d_proof + x.off_al);
    x.d_top = (uint64_t *)(run->d_proof + x.off_top);
    fs_init_kernel<<<1, 64, 0, ctx->stream>>>(x.d_fs, fs0, (const uint8_t *)rq.ride_src, run->d_proof + x.off_ride,
                                              x.back_len - x.off_ride);
    return SMI_OK;
}

// part 2: the rounds of Fri::commit (src/fri.rs:116-148), as the round plan says (fri_plan.h).  A round's codeword is read
// from memory, or computed by the launch that hashes it (LeafSrc, internal.h; the codeword buffer is written by that launch
// and everything downstream reads it as before), or folded inside the tail launch.
static int fri_rounds(FriExec &x) {
    smi_ctx *ctx = x.ctx;
    smi_fri_run *run = x.run;
    const FriRoundPlan &plan = x.plan;
    const uint32_t R = plan.R, inv2_m = fri_inv2_m(ctx);
    uint32_t omega = (uint32_t)x.rq->cfg->omega, offset = (uint32_t)x.rq->cfg->offset;
    // phase != 0: the merkle launches get no Fiat-Shamir hook (fs_words == nullptr), a phase-aware kernel follows each tree
    uint32_t *const hook_fs = x.phase == 0 ? x.d_fs->s : nullptr;
    FriTailArgs ta;   // every round from plan.tail_at on, in one workgroup launch (hash.hip, fri_tail_kernel)
    if (plan.tail_at < R) {
        memset(&ta, 0, sizeof ta);
        ta.n_rounds = R - plan.tail_at;
        ta.fs_words = x.d_fs->s;
        ta.F = ctx->fs.F;
        ta.inv2_m = inv2_m;
    }
    LeafSrc pending;   // how the launch that hashes this round's leaves computes them
    bool have_pending = x.rq->round0_src != nullptr;
    if (have_pending) pending = *x.rq->round0_src;
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t *cur = run->codewords[r];
        const uint64_t len = run->lens[r];
        const bool last = r == R - 1;
        // leaf hashes + tree (src/fri.rs:118-127); power-of-two lengths never need padding
        uint8_t *nodes = run_tree(run, len);
        if (!nodes) return smi_fail(ctx, SMI_ERR_OOM, "alloc tree");
        uint8_t *slot = run->d_proof + 33 * r;
        uint64_t *alpha_out = last ? nullptr : x.d_alphas + r;   // no challenge after the last root (src/fri.rs:133-135)
        FriTailRound *tr = plan.tree[r] == FRI_TREE_TAIL ? &ta.r[r - plan.tail_at] : nullptr;
        if (tr) {
            // the tail holds one x^-1 table per fold until its launch: none of them may be evicted in between
            if (r == plan.tail_at) SMI_TRY(ctx_scale_reserve(ctx, (size_t)(R - r)));
            tr->cw = cur;
            tr->len = (uint32_t)len;
            tr->nodes = nodes;
            tr->proof_slot = slot;
            tr->alpha_out = alpha_out;
        } else {
            // push root, absorb, challenge (src/fri.rs:129-138): done by the workgroup that finishes the tree
            // when that is the chunk kernel (one launch fewer per round), by a kernel of its own otherwise
            bool fs_done = false;
            if (have_pending) SMI_TRY(launch_merkle_src_fs(ctx, pending, len, nodes, hook_fs, slot, alpha_out, &fs_done));
            else SMI_TRY(launch_merkle_fs(ctx, cur, len, nodes, hook_fs, slot, alpha_out, &fs_done));
            have_pending = false;
            if (!fs_done) SMI_TRY(launch_fs_round(ctx, x.d_fs, nodes + (2 * len - 2) * 32, slot, alpha_out, x.phase));
        }
        if (last) break;
        const uint64_t half = len / 2;
        uint32_t *next = run_codeword(run, half);
        if (!next) return smi_fail(ctx, SMI_ERR_OOM, "alloc codeword");
        ScaleTables S;
        SMI_TRY(fri_fold_tables(ctx, offset, omega, len, &S));
        switch (plan.producer[r + 1]) {
        case FRI_BY_FOLD:
            SMI_TRY(launch_fold_tables(ctx, cur, cur + half, half, 0, x.d_alphas + r, S, inv2_m, next));
            break;
        case FRI_BY_LEAF_QUAD:   // four elements per access.  Round 1 was planned from the caller's pointer and every later buffer
            assert((((uintptr_t)cur | (uintptr_t)next) & 15u) == 0);   // is the arena's or hipMalloc's: this can only be a library bug
            [[fallthrough]];
        case FRI_BY_LEAF_CHUNK:
            memset(&pending, 0, sizeof pending);
            pending.kind = LEAF_FOLD;
            pending.cw_out = next;
            pending.F = ctx->fs.F;
            pending.lo = cur;
            pending.hi = cur + half;
            pending.alpha = x.d_alphas + r;
            pending.inv2_m = inv2_m;
            pending.S = S;
            have_pending = true;
            break;
        case FRI_BY_TAIL_HEAD:
            ta.pre_lo = cur;
            ta.pre_hi = cur + half;
            ta.pre_alpha = x.d_alphas + r;
            ta.pre_S = S;
            break;
        default:   // FRI_IN_TAIL
            tr->next = next;
            tr->S = S;
        }
        omega = h_mul(ctx, omega, omega);    // src/fri.rs:146-147
        offset = h_mul(ctx, offset, offset);
    }
    if (plan.tail_at < R) SMI_TRY(launch_fri_tail(ctx, ta));
    return SMI_OK;
}

// part 3: the last codeword in the clear, the query phase of Fri::prove, and the one synchronising copy-back
static int fri_finish(FriExec &x, FriResult *res) {
    smi_ctx *ctx = x.ctx;
    smi_fri_run *run = x.run;
    const FriLayout &lay = x.lay;
    const uint64_t R = lay.R, t = x.rq->cfg->num_colinearity_tests, len = x.rq->len;
    std::vector<LayerInfo> layers(R - 1);   // lives past the synchronisation below: the source of an asynchronous copy
    SMI_TRY(launch_emit_codeword(ctx, run->codewords[R - 1], lay.last_n, run->d_proof + lay.off_last));   // src/fri.rs:151
    if (x.rq->do_query) {
        SMI_TRY(launch_fs_challenge(ctx, x.d_fs, x.d_seed_ch, x.phase));
        const uint64_t sample_size = R > 1 ? len / 2 : len;  // src/fri.rs:266-270
        SMI_TRY(launch_sample_indices(ctx, x.d_seed_ch, sample_size, lay.last_n, (uint32_t)t, x.d_top, x.d_reduced));
        if (R > 1 && t > 0) {
            for (uint64_t i = 0; i + 1 < R; i++) {
                LayerInfo &L = layers[i];
                L.cw = run->codewords[i];
                L.cw_next = run->codewords[i + 1];
                L.nodes = run->trees[i];
                L.nodes_next = run->trees[i + 1];
                L.len = len >> i;
                L.off_triples = lay.off_triples[i];
                L.off_paths = lay.off_paths[i];
                L.depth = ilog2(L.len);
                L.depth_next = L.depth - 1;
            }
            const dim3 grid((uint32_t)t, (uint32_t)(R - 1));
            if (R - 1 <= SMI_QUERY_TAB_MAX) {   // the layer table travels as a kernel argument while it fits
                LayerTable tab;
                memset(&tab, 0, sizeof tab);
                memcpy(tab.l, layers.data(), sizeof(LayerInfo) * (R - 1));
                query_tab_kernel<<<grid, 64, 0, ctx->stream>>>(tab, x.d_top, (uint32_t)t, run->d_proof);
            } else {
                HIP_TRY(ctx, hipMemcpyAsync(x.d_layers, layers.data(), sizeof(LayerInfo) * (R - 1), hipMemcpyHostToDevice, ctx->stream));
                query_kernel<<<grid, 64, 0, ctx->stream>>>(x.d_layers, x.d_top, (uint32_t)t, run->d_proof);
            }
        }
    }
    if (hipGetLastError() != hipSuccess) return smi_fail(ctx, SMI_ERR_HIP, "fri kernel launch");

    // through the context's pinned landing buffer: proof | challenges | indices | ride-along
    uint8_t *land = nullptr;
    SMI_TRY(ctx_pin_out(ctx, x.back_len, &land));
    HIP_TRY(ctx, hipMemcpyAsync(land, run->d_proof, x.back_len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    res->lay = lay;
    res->proof.assign(land, land + lay.proof_len);
    res->alphas.assign(R, 0);
    res->top.assign(t + 1, 0);
    if (R > 1) memcpy(res->alphas.data(), land + x.off_al, 8 * (R - 1));
    if (x.rq->do_query && t) memcpy(res->top.data(), land + x.off_top, 8 * t);
    if (x.back_len > x.off_ride && x.rq->ride_dst) memcpy(x.rq->ride_dst, land + x.off_ride, x.back_len - x.off_ride);
    return SMI_OK;
}

int fri_run(smi_ctx *ctx, const FriRequest &rq, FriResult *res) {
    ScaleScope pin__(ctx);   // the fused tail collects one x^-1 table per fold before its single launch
    FriExec x;
    x.ctx = ctx, x.rq = &rq, x.run = nullptr;
    int rc = fri_setup(x);
    if (rc == SMI_OK) rc = fri_rounds(x);
    if (rc == SMI_OK) rc = fri_finish(x, res);
    if (rc == SMI_OK && rq.retain) res->run = x.run;
    else smi_fri_run_free(x.run);
    return rc;
}

// ------------------------------------------------------------------------- FRI over the quartic extension
// The round of hash_core.h fs_round_ext_lane on four lanes, one coordinate of alpha each; lane 3 keeps the state.  The
// last round (alpha_out == nullptr) absorbs its root and draws nothing.  Any phase.
__global__ __launch_bounds__(64) void fs_round_ext_kernel(FsSeed *fs, const uint32_t *root, uint8_t *proof_slot, uint64_t *alpha_out) {
    if (blockIdx.x || threadIdx.x >= 4) return;
    uint32_t m[8], in[16], out[16];
    for (int j = 0; j < 8; j++) m[j] = root[j];
    for (int j = 0; j < 16; j++) in[j] = fs->s[j];
    const uint32_t phase = fs->phase;
    if (threadIdx.x == 0) {
        proof_slot[0] = 0;
        for (int i = 0; i < 32; i++) proof_slot[1 + i] = (uint8_t)(m[i >> 2] >> (8 * (i & 3)));
    }
    if (!alpha_out) {
        if (threadIdx.x == 0) hashc::fs_absorb_root_phase(fs->s, m, phase, nullptr, nullptr);
        return;
    }
    uint64_t a;
    hashc::fs_round_ext_lane(in, m, phase, (int)threadIdx.x, out, &a);
    alpha_out[threadIdx.x] = a;
    if (threadIdx.x == 3)
        for (int j = 0; j < 16; j++) fs->s[j] = out[j];
}

// the last codeword in the clear: tag 2, count 4 len, element i at values 4 i .. 4 i + 3
__global__ void emit_codeword_ext_kernel(const uint32_t *cw, size_t stride, uint64_t len, uint8_t *dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        dst[0] = 2;
        put_u64(dst + 1, 4 * len);
    }
    if (i < 4 * len) put_u64(dst + 9 + 8 * i, cw[(i & 3) * stride + (i >> 2)]);
}

// query_one for four-column codewords: per (layer, test) one record of 12 values -- a, b, c, four coordinates each --
// and the three paths of the reference's order
struct LayerInfoExt {
    const uint32_t *cw, *cw_next;
    size_t stride, stride_next;
    const uint8_t *nodes, *nodes_next;
    uint64_t len, off_triples, off_paths;
    uint32_t depth, depth_next;
};
struct LayerTableExt {
    LayerInfoExt l[SMI_QUERY_TAB_MAX];
};
__global__ void query_ext_kernel(const LayerTableExt tab, const uint64_t *top, uint8_t *proof) {
    const LayerInfoExt &L = tab.l[blockIdx.y];
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint64_t half = L.len / 2;
    const uint64_t c = top[s] % half;
    uint8_t *tr = proof + L.off_triples + (uint64_t)s * (9 + 96);
    if (lane == 0) {
        tr[0] = 2;
        put_u64(tr + 1, 12);
    }
    if (lane < 12) {
        const uint32_t e = lane & 3, which = lane >> 2;
        const uint32_t v = which == 0 ? L.cw[e * L.stride + c] : (which == 1 ? L.cw[e * L.stride + c + half] : L.cw_next[e * L.stride_next + c]);
        put_u64(tr + 9 + 8 * lane, v);
    }
    const uint64_t pa = 9 + 32ull * L.depth, pc = 9 + 32ull * L.depth_next;
    uint8_t *pp = proof + L.off_paths + (uint64_t)s * (2 * pa + pc);
    write_path(pp, L.nodes, L.len, L.depth, c, lane);
    write_path(pp + pa, L.nodes, L.len, L.depth, c + half, lane);
    write_path(pp + 2 * pa, L.nodes_next, half, L.depth_next, c, lane);
}

// ------------------------------------------------------------------------- proof-of-work search ("Grinding")
// The smallest nonce nu whose hash with the transcript has `bits` low zero bits in its check word (hash_core.h grind_pair:
// two nonces per lane in the paired-lane state, 9 or 10 mixes each, no memory traffic and no LDS).  Round r of a lane tests
// r S + 2 gid and r S + 2 gid + 1, S = twice the lanes of the grid; a hit is published with an atomic minimum on *best
// (preset to all-ones), and before each round the lane reads *best with a relaxed agent-scope load.
//   - No workgroup ever waits for another: every lane only runs its own bounded loop, so nothing can hang.
//   - Only the value itself is communicated, so no fence is needed: a stale read costs one more round, never a wrong answer.
//   - The minimum is exact: a lane stops only below a value that is itself a valid nonce, or after its own hit, below
//     which it has tested every nonce it owns.
//   - The loop is bounded by max_tries.
__global__ __launch_bounds__(256, 8) void grind_kernel(const FsSeed *__restrict__ fs, uint32_t bits, uint64_t max_tries, unsigned long long *best) {
    uint32_t mid[16];
#pragma unroll
    for (int i = 0; i < 16; i++) mid[i] = fs->s[i];
    const uint32_t phase = fs->phase;   // uniform over the launch
    const uint64_t S = 2ull * gridDim.x * blockDim.x;
    uint64_t n = 2ull * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    for (;;) {
        const uint64_t seen = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint64_t hit;
        const bool done = hashc::grind_round(mid, phase, bits, max_tries, n, seen, &hit);
        if (hit != ~0ull) atomicMin(best, (unsigned long long)hit);
        if (done || max_tries - n <= S) break;   // (not done: n < max_tries)
        n += S;
    }
}
// One lane after the search: the nonce record (tag 2, count 1, the u64) into the proof, the nonce absorbed into the device
// transcript (its phase moves by 8), and the nonce and an "exhausted" flag (*best still all-ones) into the block that the
// prove copies back anyway.
__global__ void grind_finish_kernel(FsSeed *fs, const unsigned long long *best, uint8_t *record, uint64_t *back) {
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t nu = *best;
    record[0] = 2;
    put_u64(record + 1, 1);
    put_u64(record + 9, nu);
    back[0] = nu;
    back[1] = nu == ~0ull ? 1u : 0u;
    hashc::State st;
    for (int i = 0; i < 16; i++) st.s[i] = fs->s[i];
    uint8_t nb[8];
    for (int i = 0; i < 8; i++) nb[i] = (uint8_t)(nu >> (8 * i));
    const uint32_t k = hashc::fs_absorb_bytes_phase(st, fs->phase, nb, 8);
    for (int i = 0; i < 16; i++) fs->s[i] = st.s[i];
    fs->phase = k;
}
int grind_bits_check(smi_ctx *ctx, uint32_t bits) {
    if (bits > SMI_GRIND_MAX_BITS) return smi_fail(ctx, SMI_ERR_BAD_ARG, "grind_bits must be at most SMI_GRIND_MAX_BITS (32)");
    return SMI_OK;
}
// *d_best = all-ones, then the search over the nonces 0 .. max_tries - 1 (0: the default cap 2^(bits+6)).  The grid covers
// about 2^bits nonces per round -- the expected place of the first hit -- between one workgroup and a chip's worth (8
// workgroups of 256 per CU, the shape of the other hash kernels), and never more lanes than there are nonces to try.
static int launch_grind(smi_ctx *ctx, const FsSeed *d_fs, uint32_t bits, uint64_t max_tries, unsigned long long *d_best) {
    if (!max_tries) max_tries = 1ull << (bits + 6);
    HIP_TRY(ctx, hipMemsetAsync(d_best, 0xFF, 8, ctx->stream));
    uint64_t lanes = ((1ull << bits) + 1) / 2;
    if (lanes > max_tries / 2 + 1) lanes = max_tries / 2 + 1;
    uint64_t blocks = (lanes + 255) / 256;
    const uint64_t chip = 8ull * (uint64_t)ctx->num_cus;
    if (blocks > chip) blocks = chip;
    ProfScope ps(ctx, "grind_kernel", 0.0);
    grind_kernel<<<(uint32_t)blocks, 256, 0, ctx->stream>>>(d_fs, bits, max_tries, d_best);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int fri_run_ext(smi_ctx *ctx, const smi_fri_cfg *cfg, const FsSeed *seed, const uint32_t *d_codeword, size_t len, size_t stride, bool reset_arena,
                FriExtResult *res, int grind) {
    SMI_TRY(ext_field_check(ctx));
    SMI_TRY(smi_fri_check(ctx, cfg));
    if (cfg->domain_length != len) return smi_fail(ctx, SMI_ERR_CODEWORD_LEN, "initial codeword length does not match domain length");
    if (stride < len || len > ((size_t)1 << 27)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fri_prove_ext: stride < len, or len > 2^27");
    const uint32_t p = ctx->fs.F.p;
    if (cfg->omega >= p || cfg->offset >= p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "omega/offset must be < p");
    const bool pow = grind != SMI_GRIND_NONE;
    if (pow) SMI_TRY(grind_bits_check(ctx, (uint32_t)grind));
    const FriLayout lay = fri_layout_ext(*cfg, pow);
    const uint64_t R = lay.R, t = cfg->num_colinearity_tests;
    if (R == 0) return smi_fail(ctx, SMI_ERR_NO_ROUNDS, "num_rounds() == 0: the reference's verify rejects such a proof");
    if (R - 1 > SMI_QUERY_TAB_MAX) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fri_prove_ext: too many rounds");
    if (t > 2 * lay.last_n) return smi_fail(ctx, SMI_ERR_SAMPLE_ENTROPY, "not enough entropy in indices wrt last codeword");
    if (t > lay.last_n) return smi_fail(ctx, SMI_ERR_SAMPLE_TOO_MANY, "cannot sample more indices than available in last codeword");
    const FsSeed fs0 = seed ? *seed : fresh_seed();
    if (reset_arena) SMI_TRY(arena_reset(ctx));
    ScaleScope pin__(ctx);

    // one device buffer comes back in one copy: proof | top-level indices (| nonce, exhausted flag); beside it: fs state |
    // seed challenge | reduced | the search's best nonce
    const size_t off_top = (lay.proof_len + 7) & ~(size_t)7, off_pow = off_top + 8 * (t + 1), back_len = off_pow + (pow ? 16 : 0);
    const size_t m_alpha = (sizeof(FsSeed) + 63) & ~(size_t)63, m_seed_ch = m_alpha + 32 * R, m_reduced = m_seed_ch + 8;
    const size_t m_best = m_reduced + 8 * (t + 1);
    uint8_t *misc = (uint8_t *)arena_alloc(ctx, m_best + (pow ? 8 : 0));
    uint8_t *d_proof = (uint8_t *)arena_alloc(ctx, back_len);
    if (!misc || !d_proof) return smi_fail(ctx, SMI_ERR_OOM, "fri_prove_ext: device memory");
    FsSeed *d_fs = (FsSeed *)misc;
    uint64_t *d_alphas = (uint64_t *)(misc + m_alpha), *d_seed_ch = (uint64_t *)(misc + m_seed_ch), *d_reduced = (uint64_t *)(misc + m_reduced);
    uint64_t *d_top = (uint64_t *)(d_proof + off_top);
    fs_init_kernel<<<1, 64, 0, ctx->stream>>>(d_fs, fs0);

    LayerTableExt tab;
    memset(&tab, 0, sizeof tab);
    const uint32_t *cur = d_codeword;
    size_t cur_stride = stride;
    uint32_t omega = (uint32_t)cfg->omega, offset = (uint32_t)cfg->offset;
    for (uint64_t r = 0; r < R; r++) {
        const uint64_t n = len >> r;
        const bool last = r == R - 1;
        uint8_t *nodes = (uint8_t *)arena_alloc(ctx, (2 * n - 1) * 32);
        if (!nodes) return smi_fail(ctx, SMI_ERR_OOM, "fri_prove_ext: tree");
        SMI_TRY(launch_merkle_rows(ctx, cur, 4, cur_stride, n, nodes));   // leaf i = the hash of element i's four coordinates
        fs_round_ext_kernel<<<1, 64, 0, ctx->stream>>>(d_fs, (const uint32_t *)(nodes + (2 * n - 2) * 32), d_proof + 33 * r, last ? nullptr : d_alphas + 4 * r);
        HIP_TRY(ctx, hipGetLastError());
        if (r > 0) {
            LayerInfoExt &L = tab.l[r - 1];
            L.cw_next = cur;
            L.stride_next = cur_stride;
            L.nodes_next = nodes;
        }
        if (last) break;
        LayerInfoExt &L = tab.l[r];
        L.cw = cur;
        L.stride = cur_stride;
        L.nodes = nodes;
        L.len = n;
        L.off_triples = lay.off_triples[r];
        L.off_paths = lay.off_paths[r];
        L.depth = ilog2(n);
        L.depth_next = L.depth - 1;
        const uint64_t half = n / 2;
        uint32_t *next = (uint32_t *)arena_alloc(ctx, 16 * half);
        if (!next) return smi_fail(ctx, SMI_ERR_OOM, "fri_prove_ext: codeword");
        SMI_TRY(launch_fold_ext(ctx, cur, n, cur_stride, d_alphas + 4 * r, offset, omega, next, half));
        cur = next;
        cur_stride = half;
        omega = h_mul(ctx, omega, omega);
        offset = h_mul(ctx, offset, offset);
    }
    emit_codeword_ext_kernel<<<(uint32_t)((4 * lay.last_n + 255) / 256), 256, 0, ctx->stream>>>(cur, cur_stride, lay.last_n, d_proof + lay.off_last);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t seed_phase = fs0.phase;
    if (pow) {   // the search, then one lane writes the record and absorbs the nonce: the transcript stays on the device
        unsigned long long *d_best = (unsigned long long *)(misc + m_best);
        SMI_TRY(launch_grind(ctx, d_fs, (uint32_t)grind, 0, d_best));
        grind_finish_kernel<<<1, 64, 0, ctx->stream>>>(d_fs, d_best, d_proof + lay.off_layers - SMI_GRIND_RECORD_BYTES, (uint64_t *)(d_proof + off_pow));
        HIP_TRY(ctx, hipGetLastError());
        seed_phase = (fs0.phase + 8) & 31u;
    }
    SMI_TRY(launch_fs_challenge(ctx, d_fs, d_seed_ch, seed_phase));
    SMI_TRY(launch_sample_indices(ctx, d_seed_ch, R > 1 ? len / 2 : len, lay.last_n, (uint32_t)t, d_top, d_reduced));
    if (R > 1 && t > 0) {
        query_ext_kernel<<<dim3((uint32_t)t, (uint32_t)(R - 1)), 64, 0, ctx->stream>>>(tab, d_top, d_proof);
        HIP_TRY(ctx, hipGetLastError());
    }
    uint8_t *land = nullptr;
    SMI_TRY(ctx_pin_out(ctx, back_len, &land));
    HIP_TRY(ctx, hipMemcpyAsync(land, d_proof, back_len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (pow) {
        uint64_t back[2];
        memcpy(back, land + off_pow, 16);
        if (back[1]) return smi_fail(ctx, SMI_ERR_GRIND_EXHAUSTED, "proof of work: no nonce below 2^(grind_bits + 6) meets the difficulty");
        res->nonce = back[0];
    }
    res->proof.assign(land, land + lay.proof_len);
    res->top.assign(t + 1, 0);
    if (t) memcpy(res->top.data(), land + off_top, 8 * t);
    return SMI_OK;
}

int smi_dev_fri_prove_ext(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_codeword,
                          size_t len, size_t stride, uint8_t **proof, size_t *proof_len, uint64_t *top_indices) {
    if (!ctx || !cfg || !d_codeword || !proof || !proof_len || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    FsSeed seed;
    hashc::fs_seed(transcript, transcript_len, seed.s, &seed.phase);
    DeviceGuard dg__(ctx);
    FriExtResult res;
    SMI_TRY(fri_run_ext(ctx, cfg, &seed, d_codeword, len, stride, true, &res));
    if (top_indices) memcpy(top_indices, res.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    return smi_proof_out(ctx, res.proof, proof, proof_len);
}

int smi_dev_fri_prove_ext_pow(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_codeword,
                              size_t len, size_t stride, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, uint32_t grind_bits,
                              uint64_t *nonce) {
    if (!ctx || !cfg || !d_codeword || !proof || !proof_len || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    FsSeed seed;
    hashc::fs_seed(transcript, transcript_len, seed.s, &seed.phase);
    DeviceGuard dg__(ctx);
    FriExtResult res;
    SMI_TRY(fri_run_ext(ctx, cfg, &seed, d_codeword, len, stride, true, &res, (int)grind_bits));
    if (top_indices) memcpy(top_indices, res.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    if (nonce) *nonce = res.nonce;
    return smi_proof_out(ctx, res.proof, proof, proof_len);
}

// ------------------------------------------------------------------------- extension FRI at folding factor 4
// (include/stark_mi.h, "Extension FRI, folding factor 4").  A sibling of fri_run_ext, which stays as it is: F + 1 codewords
// of lengths N / 4^r, each committed by a tree of coset leaves (leaf i = the 16 coordinates of elements i, i + q, i + 2 q,
// i + 3 q: launch_merkle_rows over the codeword read as 16 columns q apart), one fold4 launch between two of them, the
// nonce always searched.  Per (test, layer) the query kernel writes one coset record and one path.
struct LayerInfoFold4 {
    const uint32_t *cw;      // columns 4 q apart
    const uint8_t *nodes;    // the tree of q leaves
    uint64_t q, off_cosets, off_paths;
    uint32_t depth;          // log2 q
};
struct LayerTableFold4 {
    LayerInfoFold4 l[SMI_FRI_MAX_ROUNDS / 2];
};
__global__ void query_fold4_kernel(const LayerTableFold4 tab, const uint64_t *top, uint8_t *proof) {
    const LayerInfoFold4 &L = tab.l[blockIdx.y];
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint64_t i = top[s] % L.q;
    uint8_t *rec = proof + L.off_cosets + (uint64_t)s * (9 + 128);
    if (lane == 0) {
        rec[0] = 2;
        put_u64(rec + 1, 16);
    }
    if (lane < 16) put_u64(rec + 9 + 8 * lane, L.cw[(uint64_t)lane * L.q + i]);   // lane = 4 e + j: coordinate e of element i + j q
    write_path(proof + L.off_paths + (uint64_t)s * (9 + 32ull * L.depth), L.nodes, L.q, L.depth, i, lane);
}

int fri_run_ext_fold4(smi_ctx *ctx, const smi_fri_cfg *cfg, const FsSeed *seed, const uint32_t *d_codeword, size_t len, size_t stride, bool reset_arena,
                      FriExtResult *res, uint32_t grind_bits) {
    SMI_TRY(ext_field_check(ctx));
    SMI_TRY(smi_fri_check(ctx, cfg));
    if (cfg->domain_length != len) return smi_fail(ctx, SMI_ERR_CODEWORD_LEN, "initial codeword length does not match domain length");
    if (stride < len || len > ((size_t)1 << 27)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fri_prove_ext_fold4: stride < len, or len > 2^27");
    const uint32_t p = ctx->fs.F.p;
    if (cfg->omega >= p || cfg->offset >= p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "omega/offset must be < p");
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    const FriFold4Layout lay = fri_layout_fold4(*cfg);
    const uint64_t F = lay.F, t = cfg->num_colinearity_tests;
    if (lay.R2 == 0) return smi_fail(ctx, SMI_ERR_NO_ROUNDS, "num_rounds() == 0: the reference's verify rejects such a proof");
    if (t > 2 * lay.last_n) return smi_fail(ctx, SMI_ERR_SAMPLE_ENTROPY, "not enough entropy in indices wrt last codeword");
    if (t > lay.last_n) return smi_fail(ctx, SMI_ERR_SAMPLE_TOO_MANY, "cannot sample more indices than available in last codeword");
    if (len < 4) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fri_prove_ext_fold4: a coset leaf needs four elements");
    const FsSeed fs0 = seed ? *seed : fresh_seed();
    if (reset_arena) SMI_TRY(arena_reset(ctx));
    ScaleScope pin__(ctx);

    // what comes back in one copy: proof | top-level indices | nonce, exhausted flag; beside it: fs state | alphas | seed
    // challenge | reduced | the search's best nonce
    const size_t off_top = (lay.proof_len + 7) & ~(size_t)7, off_pow = off_top + 8 * (t + 1), back_len = off_pow + 16;
    const size_t m_alpha = (sizeof(FsSeed) + 63) & ~(size_t)63, m_seed_ch = m_alpha + 32 * (F + 1), m_reduced = m_seed_ch + 8;
    const size_t m_best = m_reduced + 8 * (t + 1);
    uint8_t *misc = (uint8_t *)arena_alloc(ctx, m_best + 8);
    uint8_t *d_proof = (uint8_t *)arena_alloc(ctx, back_len);
    if (!misc || !d_proof) return smi_fail(ctx, SMI_ERR_OOM, "fri_prove_ext_fold4: device memory");
    FsSeed *d_fs = (FsSeed *)misc;
    uint64_t *d_alphas = (uint64_t *)(misc + m_alpha), *d_seed_ch = (uint64_t *)(misc + m_seed_ch), *d_reduced = (uint64_t *)(misc + m_reduced);
    uint64_t *d_top = (uint64_t *)(d_proof + off_top);
    fs_init_kernel<<<1, 64, 0, ctx->stream>>>(d_fs, fs0);

    // A coset leaf reads its codeword as 16 columns q apart, which needs the four coordinate columns exactly len apart.  A
    // caller's strided first codeword is compacted once (16 N bytes moved, against the 16 N the first tree reads anyway);
    // every later codeword is allocated here with stride == length.
    const uint32_t *cur = d_codeword;
    if (stride != len) {
        uint32_t *packed = (uint32_t *)arena_alloc(ctx, 16 * len);
        if (!packed) return smi_fail(ctx, SMI_ERR_OOM, "fri_prove_ext_fold4: codeword");
        HIP_TRY(ctx, hipMemcpy2DAsync(packed, 4 * len, d_codeword, 4 * stride, 4 * len, 4, hipMemcpyDeviceToDevice, ctx->stream));
        cur = packed;
    }
    LayerTableFold4 tab;
    memset(&tab, 0, sizeof tab);
    uint32_t omega = (uint32_t)cfg->omega, offset = (uint32_t)cfg->offset;
    for (uint64_t r = 0; r <= F; r++) {
        const uint64_t n = len >> (2 * r), q = n / 4;
        const bool last = r == F;
        uint8_t *nodes = (uint8_t *)arena_alloc(ctx, (2 * q - 1) * 32);
        if (!nodes) return smi_fail(ctx, SMI_ERR_OOM, "fri_prove_ext_fold4: tree");
        SMI_TRY(launch_merkle_rows(ctx, cur, 16, q, q, nodes));
        fs_round_ext_kernel<<<1, 64, 0, ctx->stream>>>(d_fs, (const uint32_t *)(nodes + (2 * q - 2) * 32), d_proof + 33 * r, last ? nullptr : d_alphas + 4 * r);
        HIP_TRY(ctx, hipGetLastError());
        if (last) break;
        LayerInfoFold4 &L = tab.l[r];
        L.cw = cur;
        L.nodes = nodes;
        L.q = q;
        L.off_cosets = lay.off_cosets[r];
        L.off_paths = lay.off_paths[r];
        L.depth = ilog2(q);
        uint32_t *next = (uint32_t *)arena_alloc(ctx, 16 * q);
        if (!next) return smi_fail(ctx, SMI_ERR_OOM, "fri_prove_ext_fold4: codeword");
        SMI_TRY(launch_fold4_ext(ctx, cur, n, n, d_alphas + 4 * r, offset, omega, next, q));
        cur = next;
        omega = h_pow(ctx, omega, 4);
        offset = h_pow(ctx, offset, 4);
    }
    emit_codeword_ext_kernel<<<(uint32_t)((4 * lay.last_n + 255) / 256), 256, 0, ctx->stream>>>(cur, lay.last_n, lay.last_n, d_proof + lay.off_last);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long *d_best = (unsigned long long *)(misc + m_best);
    SMI_TRY(launch_grind(ctx, d_fs, grind_bits, 0, d_best));
    grind_finish_kernel<<<1, 64, 0, ctx->stream>>>(d_fs, d_best, d_proof + lay.off_nonce, (uint64_t *)(d_proof + off_pow));
    HIP_TRY(ctx, hipGetLastError());
    SMI_TRY(launch_fs_challenge(ctx, d_fs, d_seed_ch, (fs0.phase + 8) & 31u));
    SMI_TRY(launch_sample_indices(ctx, d_seed_ch, F ? len / 4 : len, lay.last_n, (uint32_t)t, d_top, d_reduced));
    if (F && t > 0) {
        query_fold4_kernel<<<dim3((uint32_t)t, (uint32_t)F), 64, 0, ctx->stream>>>(tab, d_top, d_proof);
        HIP_TRY(ctx, hipGetLastError());
    }
    uint8_t *land = nullptr;
    SMI_TRY(ctx_pin_out(ctx, back_len, &land));
    HIP_TRY(ctx, hipMemcpyAsync(land, d_proof, back_len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t back[2];
    memcpy(back, land + off_pow, 16);
    if (back[1]) return smi_fail(ctx, SMI_ERR_GRIND_EXHAUSTED, "proof of work: no nonce below 2^(grind_bits + 6) meets the difficulty");
    res->nonce = back[0];
    res->proof.assign(land, land + lay.proof_len);
    res->top.assign(t + 1, 0);
    if (t) memcpy(res->top.data(), land + off_top, 8 * t);
    return SMI_OK;
}

int smi_dev_fri_prove_ext_fold4(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_codeword,
                                size_t len, size_t stride, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, uint32_t grind_bits,
                                uint64_t *nonce) {
    if (!ctx || !cfg || !d_codeword || !proof || !proof_len || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    FsSeed seed;
    hashc::fs_seed(transcript, transcript_len, seed.s, &seed.phase);
    DeviceGuard dg__(ctx);
    FriExtResult res;
    SMI_TRY(fri_run_ext_fold4(ctx, cfg, &seed, d_codeword, len, stride, true, &res, grind_bits));
    if (top_indices) memcpy(top_indices, res.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    if (nonce) *nonce = res.nonce;
    return smi_proof_out(ctx, res.proof, proof, proof_len);
}

// pow_ok on the host: the definition as it stands, one Hash::from_bytes of transcript || nonce
int smi_grind_check(const uint8_t *transcript, size_t transcript_len, uint64_t nonce, uint32_t bits, int *ok) {
    if (!ok || (!transcript && transcript_len) || bits > SMI_GRIND_MAX_BITS) return SMI_ERR_BAD_ARG;
    std::vector<uint8_t> msg(transcript_len + 8);
    if (transcript_len) memcpy(msg.data(), transcript, transcript_len);
    for (int i = 0; i < 8; i++) msg[transcript_len + i] = (uint8_t)(nonce >> (8 * i));
    uint32_t d[8];
    hashc::hash_bytes(msg.data(), msg.size(), d);
    const uint64_t word = (uint64_t)d[6] | ((uint64_t)d[7] << 32);
    *ok = (word & ((1ull << bits) - 1)) == 0;
    return SMI_OK;
}

// the search alone: host transcript -> FsSeed on the device -> grind_kernel -> one synchronising copy of *best
int smi_dev_grind(smi_ctx *ctx, const uint8_t *transcript, size_t transcript_len, uint32_t bits, uint64_t max_tries, uint64_t *nonce) {
    if (!ctx || !nonce || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    SMI_TRY(grind_bits_check(ctx, bits));
    FsSeed seed;
    hashc::fs_seed(transcript, transcript_len, seed.s, &seed.phase);
    DeviceGuard dg__(ctx);
    void *d = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, 256, &d));
    FsSeed *d_fs = (FsSeed *)d;
    unsigned long long *d_best = (unsigned long long *)((uint8_t *)d + 128);
    fs_init_kernel<<<1, 64, 0, ctx->stream>>>(d_fs, seed);
    HIP_TRY(ctx, hipGetLastError());
    SMI_TRY(launch_grind(ctx, d_fs, bits, max_tries, d_best));
    uint8_t *land = nullptr;
    SMI_TRY(ctx_pin_out(ctx, 8, &land));
    HIP_TRY(ctx, hipMemcpyAsync(land, d_best, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t best;
    memcpy(&best, land, 8);
    if (best == ~0ull) return smi_fail(ctx, SMI_ERR_GRIND_EXHAUSTED, "proof of work: no nonce below max_tries meets the difficulty");
    *nonce = best;
    return SMI_OK;
}

// ------------------------------------------------------------------------- C ABI
// Accessors of a retained commit: the `codewords` Fri::commit returns (src/fri.rs:153-155) and
// MerkleTree::open on the per-round trees (src/fri.rs:297-298 rebuilds them; here they are kept).
int smi_fri_run_num_codewords(const smi_fri_run *run, size_t *n) {
    if (!run || !n) return SMI_ERR_BAD_ARG;
    *n = run->codewords.size();
    return SMI_OK;
}
int smi_fri_run_codeword(smi_fri_run *run, size_t round, uint64_t *out, size_t *len) {
    if (!run || !len) return SMI_ERR_BAD_ARG;
    if (round >= run->codewords.size()) return smi_fail(run->ctx, SMI_ERR_INDEX_OOB, nullptr);
    *len = run->lens[round];
    if (!out) return SMI_OK;
    return smi_dev_download_u64(run->ctx, run->codewords[round], run->lens[round], out);
}
int smi_fri_run_open(smi_fri_run *run, size_t round, size_t index, uint8_t *path, size_t *depth) {
    if (!run || !path || !depth) return SMI_ERR_BAD_ARG;
    if (round >= run->trees.size()) return smi_fail(run->ctx, SMI_ERR_INDEX_OOB, nullptr);
    smi_tree t{run->ctx, run->trees[round], (size_t)run->lens[round], false};
    return smi_merkle_open(run->ctx, &t, index, path, depth);
}

int smi_dev_fri_fold(smi_ctx *ctx, const uint32_t *d_in, size_t len, const uint64_t *d_alpha, uint64_t offset,
                     uint64_t omega, uint32_t *d_out) {
    if (!ctx || !d_in || !d_alpha || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return launch_fold_shard(ctx, d_in, d_in + len / 2, len / 2, 0, len, d_alpha, offset, omega, d_out);   // (it checks len)
}

// the caller's transcript (host bytes) as the device starts from it; (NULL, 0) is a fresh FiatShamir
static int transcript_seed(const uint8_t *transcript, size_t transcript_len, FsSeed *seed) {
    if (!transcript && transcript_len) return SMI_ERR_BAD_ARG;
    hashc::fs_seed(transcript, transcript_len, seed->s, &seed->phase);
    return SMI_OK;
}

int smi_dev_fri_prove_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint32_t *d_codeword,
                         size_t len, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, smi_fri_run **run) {
    if (!ctx || !cfg || !d_codeword || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    FsSeed seed;
    SMI_TRY(transcript_seed(transcript, transcript_len, &seed));
    DeviceGuard dg__(ctx);
    FriRequest rq(cfg, d_codeword, len, true);
    rq.retain = run != nullptr;
    rq.seed = &seed;
    FriResult res;
    SMI_TRY(fri_run(ctx, rq, &res));
    if (run) *run = res.run;
    if (top_indices) memcpy(top_indices, res.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    return smi_proof_out(ctx, res.proof, proof, proof_len);
}

int smi_dev_fri_prove(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint32_t *d_codeword, size_t len, uint8_t **proof,
                      size_t *proof_len, uint64_t *top_indices, smi_fri_run **run) {
    return smi_dev_fri_prove_fs(ctx, cfg, nullptr, 0, d_codeword, len, proof, proof_len, top_indices, run);
}

static int upload_codeword(smi_ctx *ctx, const uint64_t *codeword, size_t len, uint32_t **d_cw) {
    if (hipMalloc((void **)d_cw, len * 4 ? len * 4 : 4) != hipSuccess) return smi_fail(ctx, SMI_ERR_OOM, "hipMalloc codeword");
    return host_to_dev_u32(ctx, codeword, len, *d_cw, 0);
}

int smi_fri_prove_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint64_t *codeword,
                     size_t len, uint8_t **proof, size_t *proof_len, uint64_t *top_indices) {
    if (!ctx || !cfg || !codeword || !proof || !proof_len || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(smi_fri_check(ctx, cfg));
    if (cfg->domain_length != len) return smi_fail(ctx, SMI_ERR_CODEWORD_LEN, "initial codeword length does not match domain length");
    uint32_t *d_cw = nullptr;
    int rc = upload_codeword(ctx, codeword, len, &d_cw);
    if (rc == SMI_OK) rc = smi_dev_fri_prove_fs(ctx, cfg, transcript, transcript_len, d_cw, len, proof, proof_len, top_indices, nullptr);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_cw);
    return rc;
}
int smi_fri_prove(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint64_t *codeword, size_t len, uint8_t **proof,
                  size_t *proof_len, uint64_t *top_indices) {
    return smi_fri_prove_fs(ctx, cfg, nullptr, 0, codeword, len, proof, proof_len, top_indices);
}

int smi_fri_commit_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint64_t *codeword,
                      size_t len, uint8_t *roots, uint64_t *alphas, uint64_t *last_codeword, size_t *last_len, smi_fri_run **run) {
    if (!ctx || !cfg || !codeword) return SMI_ERR_BAD_ARG;
    FsSeed seed;
    SMI_TRY(transcript_seed(transcript, transcript_len, &seed));
    DeviceGuard dg__(ctx);
    SMI_TRY(smi_fri_check(ctx, cfg));
    if (cfg->domain_length != len) return smi_fail(ctx, SMI_ERR_CODEWORD_LEN, "initial codeword length does not match domain length");
    uint32_t *d_cw = nullptr;
    int rc = upload_codeword(ctx, codeword, len, &d_cw);
    FriRequest rq(cfg, d_cw, len, false);
    rq.retain = run != nullptr;
    rq.seed = &seed;
    FriResult res;
    if (rc == SMI_OK) rc = fri_run(ctx, rq, &res);
    (void)hipStreamSynchronize(ctx->stream);
    if (rc == SMI_OK) {
        const uint64_t R = res.lay.R;
        if (roots)
            for (uint64_t r = 0; r < R; r++) memcpy(roots + 32 * r, res.proof.data() + 33 * r + 1, 32);
        if (alphas) memcpy(alphas, res.alphas.data(), 8 * (R - 1));
        if (last_codeword) memcpy(last_codeword, res.proof.data() + res.lay.off_last + 9, 8 * res.lay.last_n);
        if (last_len) *last_len = res.lay.last_n;
    }
    if (rc == SMI_OK && run) {
        res.run->owns_first = true;  // the run keeps the uploaded codeword
        *run = res.run;
    } else {
        (void)hipFree(d_cw);
    }
    return rc;
}
int smi_fri_commit(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint64_t *codeword, size_t len, uint8_t *roots,
                   uint64_t *alphas, uint64_t *last_codeword, size_t *last_len, smi_fri_run **run) {
    return smi_fri_commit_fs(ctx, cfg, nullptr, 0, codeword, len, roots, alphas, last_codeword, last_len, run);
}

int smi_fri_fold(smi_ctx *ctx, const uint64_t *codeword, size_t len, uint64_t alpha, uint64_t offset, uint64_t omega,
                 uint64_t *out) {
    if (!ctx || !codeword || !out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (len < 2 || !is_pow2(len)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "fold: codeword length must be a power of two >= 2");
    void *d_in, *d_out, *d_alpha;
    SMI_TRY(ctx_tmp(ctx, 1, len * 4, &d_in));
    SMI_TRY(ctx_tmp(ctx, 2, len * 2 + 8, &d_out));
    SMI_TRY(ctx_tmp(ctx, 3, 8, &d_alpha));
    SMI_TRY(host_to_dev_u32(ctx, codeword, len, (uint32_t *)d_in, 0));
    HIP_TRY(ctx, hipMemcpyAsync(d_alpha, &alpha, 8, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t *cw = (const uint32_t *)d_in;
    SMI_TRY(launch_fold_shard(ctx, cw, cw + len / 2, len / 2, 0, len, (const uint64_t *)d_alpha, offset, omega, (uint32_t *)d_out));
    return dev_u32_to_host(ctx, (const uint32_t *)d_out, len / 2, out);
}
