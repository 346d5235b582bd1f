// deep.hip -- out-of-domain sampling (include/stark_mi.h, "Out-of-domain sampling"): coefficient columns evaluated at one or
// two points of F_q, the DEEP codeword, and the prover with its second commitment (the composition's segments) and its
// three host round trips.  The lane bodies and the host tables are deep_core.h, shared with the CPU emulator (emu_deep.cpp);
// the verifier is in verify.hip.
//
// Evaluation is a two-level reduction with no atomics (the sums are exact residues: any order gives the same words):
//   deep_eval_kernel          workgroup (b, .) takes coefficients [b T, (b + 1) T) (T = DEEP_TILE) of one column after the
//                             other; a lane holds the powers z^(4 tid .. 4 tid + 3) of both points in registers -- loaded
//                             once, reused for every column -- so a coefficient costs one 4-byte read and four base-field
//                             multiplies per point; the lanes' sums meet by wave shuffles and one LDS step;
//   deep_eval_combine_kernel  one workgroup per (column, point): sum_b partial_b (z^T)^b, a lane by Horner over every
//                             DEEP_BLOCK-th partial, then one table power and the same reduction.
// Two launches whatever the number of columns is.
//
// deep_compose_kernel streams: per lane four consecutive points, one 16-byte load per trace column and per segment
// coordinate, one 16-byte store per coordinate of Q: 4 (W + 4 D) + 16 bytes a point.  The eight denominators of a lane
// (x - z and x - z w at four points) share one F_q inversion; the constants sum gamma u are folded into two subtrahends on
// the host.  x advances by a per-lane step over a grid-stride loop.
#include <string>
#include <vector>

#include "air_core.h"
#include "deep_core.h"
#include "hash_core.h"
#include "internal.h"
#include "mgpu_core.h"
#include "row4_dev.h"
#include "xargs_core.h"
#include "zk_core.h"

// four consecutive words from `at` (a multiple of 4): one 16-byte access where the layout allows and all four lie below len
template <bool VEC>
__device__ __forceinline__ void deep_load4(const uint32_t *__restrict__ src, uint64_t at, uint64_t len, uint32_t v[4]) {
    if (VEC && at + 4 <= len) {
        const uint4 t = *(const uint4 *)(src + at);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
    }
}

// the workgroup's sum of one residue per lane -> valid in lane 0; red: DEEP_BLOCK / 64 words of LDS per call site
__device__ __forceinline__ uint32_t deep_block_sum(uint32_t v, uint32_t *red, uint32_t p) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v = fp_add(v, __shfl_down(v, off, 64), p);
    const uint32_t tid = threadIdx.x;
    if (!(tid & 63)) red[tid >> 6] = v;
    __syncthreads();
    if (!tid) {
#pragma unroll
        for (int w = 1; w < DEEP_BLOCK / 64; w++) v = fp_add(v, red[w], p);
    }
    return v;
}

// part[((c * nb + b) * NP + k) * 4 + e]: coordinate e of sum_{j < T} a_c[b T + j] z_k^j
template <bool VEC, int NP>
__global__ __launch_bounds__(DEEP_BLOCK) void deep_eval_kernel(Fp F, const uint32_t *__restrict__ cols, size_t stride, uint32_t n_cols, uint64_t n_coeffs,
                                                                const uint32_t *__restrict__ tab, uint32_t *__restrict__ part) {
    __shared__ uint32_t red[NP * 4][DEEP_BLOCK / 64];
    const uint32_t tid = threadIdx.x, nb = gridDim.x, b = blockIdx.x;
    const uint64_t at = (uint64_t)b * DEEP_TILE + DEEP_ROWS * tid;
    uint32_t tw[NP][4][DEEP_ROWS];
#pragma unroll
    for (int k = 0; k < NP; k++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint4 t = *(const uint4 *)(tab + (size_t)(k * 4 + e) * DEEP_TILE + DEEP_ROWS * tid);
            tw[k][e][0] = t.x, tw[k][e][1] = t.y, tw[k][e][2] = t.z, tw[k][e][3] = t.w;
        }
    for (uint32_t c = blockIdx.y; c < n_cols; c += gridDim.y) {   // workgroup-uniform trip count
        uint32_t a[DEEP_ROWS];
        deep_load4<VEC>(cols + (size_t)c * stride, at, n_coeffs, a);
        uint32_t acc[NP][4];
#pragma unroll
        for (int k = 0; k < NP; k++) deep_eval_lane(a, tw[k], F, acc[k]);
        __syncthreads();   // the sums of the column before are stored
#pragma unroll
        for (int k = 0; k < NP; k++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t s = deep_block_sum(acc[k][e], red[k * 4 + e], F.p);
                if (!tid) part[(((size_t)c * nb + b) * NP + k) * 4 + e] = s;
            }
    }
}

// out[(c * NP + k) * 4 + e] = coordinate e of sum_b partial_b (z_k^T)^b
template <int NP>
__global__ __launch_bounds__(DEEP_BLOCK) void deep_eval_combine_kernel(Fp F, uint32_t g_m, const uint32_t *__restrict__ part, uint32_t nb,
                                                                        const uint32_t *__restrict__ tab, uint32_t *__restrict__ out) {
    __shared__ uint32_t red[4][DEEP_BLOCK / 64];
    const uint32_t tid = threadIdx.x, c = blockIdx.x, k = blockIdx.y;
    const uint32_t *tp = tab + deep_eval_tp_at(NP) + (size_t)(k * DEEP_BLOCK + tid) * 4, *st = tab + deep_eval_st_at(NP) + 4 * k;
    const uint32_t tp_m[4] = {tp[0], tp[1], tp[2], tp[3]}, st_m[4] = {st[0], st[1], st[2], st[3]};
    uint32_t acc[4];
    deep_eval_combine_lane(part + ((size_t)c * nb * NP + k) * 4, NP * 4, nb, tid, tp_m, st_m, g_m, F, acc);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const uint32_t s = deep_block_sum(acc[e], red[e], F.p);
        if (!tid) out[((size_t)c * NP + k) * 4 + e] = s;
    }
}

// out (four coordinate columns) = Q on the N points h omega^i
template <bool VEC>
__global__ __launch_bounds__(DEEP_BLOCK) void deep_compose_kernel(Fp F, uint32_t g_m, uint32_t W, uint32_t D, uint64_t N, uint32_t h_m, uint32_t omega_m,
                                                                   const uint32_t *__restrict__ tab, const uint32_t *__restrict__ lde, size_t stride,
                                                                   const uint32_t *__restrict__ seg, size_t seg_stride, uint32_t *__restrict__ out,
                                                                   size_t out_stride) {
    const uint64_t groups = N / DEEP_ROWS, gid = (uint64_t)blockIdx.x * DEEP_BLOCK + threadIdx.x, gstep = (uint64_t)gridDim.x * DEEP_BLOCK;
    uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * DEEP_ROWS, F), F);
    const uint32_t xstep_m = mont_pow(omega_m, gstep * DEEP_ROWS, F);
    for (uint64_t g = gid; g < groups; g += gstep) {
        const uint64_t i0 = g * DEEP_ROWS;   // N is a multiple of 4: i0 + 3 < N
        uint32_t o[4][DEEP_ROWS];
        deep_compose_points(
            tab, W, D, g_m, F, x_m, omega_m, [&](uint32_t c, uint32_t v[4]) { perm_load4<VEC>(lde + (size_t)c * stride, i0, N, v); },
            [&](uint32_t col, uint32_t v[4]) { perm_load4<VEC>(seg + (size_t)col * seg_stride, i0, N, v); }, o);
#pragma unroll
        for (int e = 0; e < 4; e++) perm_store4<VEC>(out + e * out_stride, i0, N, o[e]);
        x_m = mont_mul(x_m, xstep_m, F);
    }
}

namespace {
// device bytes one evaluation wants behind its table: the partial sums
size_t deep_eval_part_bytes(uint32_t n_cols, uint64_t n_coeffs, uint32_t P) { return (size_t)n_cols * deep_eval_blocks(n_coeffs) * P * 16; }

// the two launches: d_tab = the table of deep_eval_build for exactly P points (16-byte aligned), d_part =
// deep_eval_part_bytes, d_out = n_cols * P * 4 words
int deep_eval_enqueue(smi_ctx *ctx, const uint32_t *d_cols, uint32_t n_cols, uint64_t n_coeffs, size_t stride, uint32_t P, const uint32_t *d_tab,
                      uint32_t *d_part, uint32_t *d_out) {
    const Fp F = ctx->fs.F;
    const uint32_t g_m = air_to_m(ctx->fs.g, F.p);
    const uint64_t nb = deep_eval_blocks(n_coeffs);
    const bool vec = al16(d_cols) && !(stride & 3);
    uint64_t gy = ((uint64_t)ctx->num_cus * 8 + nb - 1) / nb;   // enough workgroups to fill the device; the rest of the columns loop
    if (gy > n_cols) gy = n_cols;
    if (gy > 65535) gy = 65535;
    const dim3 grid((uint32_t)nb, (uint32_t)gy);
    {
        ProfScope ps(ctx, "deep_eval_kernel", 4.0 * (double)n_cols * (double)n_coeffs);
        if (P == 2) {
            if (vec) deep_eval_kernel<true, 2><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, d_cols, stride, n_cols, n_coeffs, d_tab, d_part);
            else deep_eval_kernel<false, 2><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, d_cols, stride, n_cols, n_coeffs, d_tab, d_part);
        } else {
            if (vec) deep_eval_kernel<true, 1><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, d_cols, stride, n_cols, n_coeffs, d_tab, d_part);
            else deep_eval_kernel<false, 1><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, d_cols, stride, n_cols, n_coeffs, d_tab, d_part);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, "deep_eval_combine_kernel", 16.0 * (double)n_cols * (double)nb * P);
        if (P == 2) deep_eval_combine_kernel<2><<<dim3(n_cols, 2), DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, d_part, (uint32_t)nb, d_tab, d_out);
        else deep_eval_combine_kernel<1><<<dim3(n_cols, 1), DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, d_part, (uint32_t)nb, d_tab, d_out);
        HIP_TRY(ctx, hipGetLastError());
    }
    return SMI_OK;
}

// d_tab: the table of deep_compose_build on the device
int deep_compose_enqueue(smi_ctx *ctx, uint32_t W, uint32_t D, uint32_t log_N, uint32_t h, const uint32_t *d_tab, const uint32_t *d_lde, size_t stride,
                         const uint32_t *d_seg, size_t seg_stride, uint32_t *d_out, size_t out_stride) {
    const Fp F = ctx->fs.F;
    const uint64_t N = 1ull << log_N;
    const bool vec = al16(d_lde) && al16(d_seg) && al16(d_out) && !(stride & 3) && !(seg_stride & 3) && !(out_stride & 3);
    const uint64_t groups = N / DEEP_ROWS, want = (groups + DEEP_BLOCK - 1) / DEEP_BLOCK, cap = (uint64_t)ctx->num_cus * 8;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint32_t g_m = air_to_m(ctx->fs.g, F.p), h_m = air_to_m(h, F.p), omega_m = air_to_m(h_root(ctx, log_N), F.p);
    ProfScope ps(ctx, "deep_compose_kernel", (4.0 * (W + 4.0 * D) + 16.0) * (double)N);
    if (vec) deep_compose_kernel<true><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, W, D, N, h_m, omega_m, d_tab, d_lde, stride, d_seg, seg_stride, d_out, out_stride);
    else deep_compose_kernel<false><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, W, D, N, h_m, omega_m, d_tab, d_lde, stride, d_seg, seg_stride, d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int deep_field_check(smi_ctx *ctx) {
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "deep: modulus must be < 2^30");
    return SMI_OK;
}
// four canonical coordinates -> the point; refused when a coordinate is >= p
int deep_point(smi_ctx *ctx, const uint64_t *v, FqH *z) {
    for (int e = 0; e < 4; e++) {
        if (v[e] >= ctx->fs.F.p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "deep: a coordinate of a point is >= p");
        z->c[e] = (uint32_t)v[e];
    }
    return SMI_OK;
}
}  // namespace

int smi_dev_poly_eval_ext(smi_ctx *ctx, const uint32_t *d_coeffs, uint32_t n_cols, size_t n_coeffs, size_t stride, const uint64_t *points,
                          uint32_t n_points, uint64_t *out) {
    if (!ctx || !d_coeffs || !points || !out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(deep_field_check(ctx));
    if (!n_cols || n_cols > 65535) return smi_fail(ctx, SMI_ERR_BAD_ARG, "poly_eval_ext: 1 .. 65535 columns");
    if (!n_coeffs || n_coeffs > ((size_t)1 << 27)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "poly_eval_ext: 1 .. 2^27 coefficients");
    if (stride < n_coeffs) return smi_fail(ctx, SMI_ERR_BAD_ARG, "poly_eval_ext: stride < n_coeffs");
    if (n_points < 1 || n_points > DEEP_MAX_POINTS) return smi_fail(ctx, SMI_ERR_BAD_ARG, "poly_eval_ext: one or two points");
    FqH z[DEEP_MAX_POINTS];
    for (uint32_t k = 0; k < n_points; k++) SMI_TRY(deep_point(ctx, points + 4 * k, &z[k]));
    std::vector<uint32_t> tab;
    deep_eval_build(ctx->fs.F, ctx->fs.g, n_points, z, &tab);
    const size_t b_tab = up16(tab.size() * 4), b_part = up16(deep_eval_part_bytes(n_cols, n_coeffs, n_points)), n_out = (size_t)n_cols * n_points * 4;
    void *base = nullptr;   // table | partial sums | results
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_part + n_out * 4, &base));
    uint32_t *d_tab = (uint32_t *)base, *d_part = (uint32_t *)((uint8_t *)base + b_tab), *d_out = (uint32_t *)((uint8_t *)base + b_tab + b_part);
    HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_eval_enqueue(ctx, d_coeffs, n_cols, n_coeffs, stride, n_points, d_tab, d_part, d_out));
    std::vector<uint32_t> res(n_out);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_out, n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n_out; i++) out[i] = res[i];
    return SMI_OK;
}

int smi_dev_deep_compose(smi_ctx *ctx, const smi_stark_cfg *cfg, uint32_t n_segments, const uint32_t *d_lde, size_t stride, const uint32_t *d_seg,
                         size_t seg_stride, const uint64_t z[4], const uint64_t *ood, const uint64_t *challenges, uint32_t *d_out, size_t out_stride) {
    if (!ctx || !cfg || !d_lde || !d_seg || !z || !ood || !challenges || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(deep_field_check(ctx));
    const uint32_t W = cfg->n_cols, D = n_segments, log_N = cfg->log_n + cfg->log_blowup;
    if (!W || W > 64) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose: 1..64 columns");
    if (!D || D > DEEP_MAX_SEGMENTS) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose: 1 .. 16 segments");
    if (cfg->log_n < 1 || cfg->log_blowup < 2 || log_N > 27) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose: log_n >= 1, log_blowup >= 2, log_n + log_blowup <= 27");
    if (log_N > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    const uint64_t N = 1ull << log_N;
    if (stride < N || seg_stride < N || out_stride < N) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose: stride < N, seg_stride < N or out_stride < N");
    if (!cfg->lde_offset || cfg->lde_offset >= ctx->fs.F.p) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose: lde_offset must be in 1 .. p-1");
    FqH zq;
    SMI_TRY(deep_point(ctx, z, &zq));
    if (fqh_in_base(zq)) return smi_fail(ctx, SMI_ERR_BAD_ARG, DEEP_Z_IN_BASE_FIELD);
    for (size_t i = 0; i < 4 * (2 * (size_t)W + D); i++)
        if (ood[i] >= ctx->fs.F.p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "deep_compose: an out-of-domain coordinate is >= p");
    std::vector<uint32_t> tab;
    deep_compose_build(ctx->fs.F, ctx->fs.g, W, D, h_root(ctx, cfg->log_n), zq, ood, challenges, &tab);
    void *d_tab = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, tab.size() * 4, &d_tab));
    HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    return deep_compose_enqueue(ctx, W, D, log_N, (uint32_t)cfg->lde_offset, (const uint32_t *)d_tab, d_lde, stride, d_seg, seg_stride, d_out, out_stride);
}

int smi_dev_air_prove_deep(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const uint32_t *d_trace_cols, uint8_t *roots_out, uint64_t *ood_out,
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    const smi_air *air = (const smi_air *)air_;
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(deep_field_check(ctx));
    uint32_t D = 0;
    {
        std::string why;
        const int rc = deep_plan(ctx->fs.F.p, cfg, air, nullptr, &D, &why);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    const uint32_t W = cfg->n_cols, K = air->n_constraints, log_n = cfg->log_n, log_N = cfg->log_n + cfg->log_blowup;
    if (log_N > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    const size_t n = (size_t)1 << log_n, N = (size_t)1 << log_N;
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, log_n);
    AirHost H;
    air_build(ctx->fs.F, h_root(ctx, log_N), cfg, air, &H);
    SMI_TRY(arena_reset(ctx));
    struct Events {   // destroyed on every return path
        hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } evs;
    const bool timed = stage_ms != nullptr;
    if (timed)
        for (int i = 0; i < 8; i++) HIP_TRY(ctx, hipEventCreate(&evs.ev[i]));
    auto mark = [&](int i) { if (timed) (void)hipEventRecord(evs.ev[i], ctx->stream); };

    const uint32_t n_ood = 4 * (2 * W + D);
    const size_t tree_bytes = 2 * N * 32, w_tab1 = deep_eval_tab_words(1), w_tab2 = deep_eval_tab_words(2);
    const size_t part_a = deep_eval_part_bytes(W, n, 2), part_b = deep_eval_part_bytes(D, n, 1);
    uint32_t *d_lde = (uint32_t *)arena_alloc(ctx, (size_t)W * N * 4);
    uint32_t *d_cw = (uint32_t *)arena_alloc(ctx, 4 * N * 4);        // H, then Q
    uint32_t *d_hc = (uint32_t *)arena_alloc(ctx, 4 * N * 4);        // the coefficients of H's coordinates
    uint32_t *d_seg = (uint32_t *)arena_alloc(ctx, 4 * (size_t)D * N * 4);
    uint32_t *d_coef = (uint32_t *)arena_alloc(ctx, (size_t)W * n * 4);
    uint64_t *d_weights = (uint64_t *)arena_alloc(ctx, 8 * 4 * (size_t)(W + K));
    uint32_t *d_blob = (uint32_t *)arena_alloc(ctx, H.blob.size() * 4);
    uint8_t *tree1 = (uint8_t *)arena_alloc(ctx, tree_bytes), *tree2 = (uint8_t *)arena_alloc(ctx, tree_bytes);
    uint32_t *d_tab2 = (uint32_t *)arena_alloc(ctx, w_tab2 * 4), *d_tab1 = (uint32_t *)arena_alloc(ctx, w_tab1 * 4);
    uint32_t *d_part = (uint32_t *)arena_alloc(ctx, part_a > part_b ? part_a : part_b);
    uint32_t *d_res = (uint32_t *)arena_alloc(ctx, (size_t)(8 * W + 16 * D) * 4);   // f_c at z and z w | H_{j,e} at z, e-major
    uint32_t *d_ctab = (uint32_t *)arena_alloc(ctx, deep_tab_words(W, D) * 4);
    uint32_t *d_ptab = nullptr, *d_pvals = nullptr;
    if (H.dev.Q) {
        d_ptab = (uint32_t *)arena_alloc(ctx, H.per.table_words * 4);
        d_pvals = (uint32_t *)arena_alloc(ctx, H.per.vals.size() * 4);
    }
    if (!d_lde || !d_cw || !d_hc || !d_seg || !d_coef || !d_weights || !d_blob || !tree1 || !tree2 || !d_tab2 || !d_tab1 || !d_part || !d_res || !d_ctab ||
        (H.dev.Q && (!d_ptab || !d_pvals)))
        return smi_fail(ctx, SMI_ERR_OOM, "air_prove_deep: device memory");
    mark(0);
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, W, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_lde));
    mark(1);
    SMI_TRY(launch_merkle_rows(ctx, d_lde, W, N, N, tree1));
    mark(2);
    // first round trip: root_1 -> the composition weights
    uint8_t roots[64];
    HIP_TRY(ctx, hipMemcpyAsync(roots, tree1 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, d_pvals, d_ptab));   // queued before the host waits for the root
    SMI_TRY(dev_ntt(ctx, d_trace_cols, d_coef, log_n, n, W, n, n, 1, cfg->trace_offset, 1));   // the trace polynomials, for step 5
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    Transcript tr;
    std::vector<uint64_t> weights, gammas;
    deep_transcript_weights(tr, roots, W, K, &weights);
    HIP_TRY(ctx, hipMemcpyAsync(d_weights, weights.data(), 8 * weights.size(), hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(air_compose_ext_launch(ctx, H, d_blob, d_lde, N, d_weights, d_cw, N));
    mark(3);
    // the segments: coefficients of every coordinate of H on the coset, D slices of n, each extended back to the N points
    SMI_TRY(dev_ntt(ctx, d_cw, d_hc, log_N, N, 4, N, N, 1, cfg->lde_offset, 1));
    for (uint32_t j = 0; j < D; j++)
        SMI_TRY(dev_ntt(ctx, d_hc + (size_t)j * n, d_seg + 4 * (size_t)j * N, log_N, n, 4, N, N, 0, cfg->lde_offset, 1));
    SMI_TRY(launch_merkle_rows(ctx, d_seg, 4 * D, N, N, tree2));
    mark(4);
    // second round trip: root_2 -> z
    HIP_TRY(ctx, hipMemcpyAsync(roots + 32, tree2 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t zr[4];
    deep_transcript_z(tr, roots + 32, W, K, zr);
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return smi_fail(ctx, SMI_ERR_BAD_ARG, DEEP_Z_IN_BASE_FIELD);
    if (roots_out) memcpy(roots_out, roots, 64);
    // third round trip: u = f(z), v = f(z w), s = H_j(z)
    const FqH pts[2] = {z, fqh_scale(z, w_n, p)};
    std::vector<uint32_t> tab2, tab1, ctab, res(8 * (size_t)W + 16 * (size_t)D);
    deep_eval_build(ctx->fs.F, g, 2, pts, &tab2);
    deep_eval_build(ctx->fs.F, g, 1, pts, &tab1);
    HIP_TRY(ctx, hipMemcpyAsync(d_tab2, tab2.data(), tab2.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_tab1, tab1.data(), tab1.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_eval_enqueue(ctx, d_coef, W, n, n, 2, d_tab2, d_part, d_res));
    for (uint32_t e = 0; e < 4; e++)   // coordinate e of the D segments: D columns of n coefficients, n apart
        SMI_TRY(deep_eval_enqueue(ctx, d_hc + (size_t)e * N, D, n, n, 1, d_tab1, d_part, d_res + 8 * (size_t)W + 4 * (size_t)e * D));
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_res, res.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> ood(n_ood);
    for (uint32_t c = 0; c < W; c++)
        for (uint32_t e = 0; e < 4; e++) ood[4 * c + e] = res[8 * c + e], ood[4 * (W + c) + e] = res[8 * c + 4 + e];
    for (uint32_t j = 0; j < D; j++) {   // s_j = sum_e X^e H_{j,e}(z)
        FqH s = fqh(0), xe = fqh(1 % p);
        const FqH X{{0, 1 % p, 0, 0}};
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t *v = &res[8 * (size_t)W + 4 * ((size_t)e * D + j)];
            s = fqh_add(s, fqh_mul(xe, FqH{{v[0], v[1], v[2], v[3]}}, p, g), p);
            xe = fqh_mul(xe, X, p, g);
        }
        for (uint32_t e = 0; e < 4; e++) ood[4 * (2 * W + j) + e] = s.c[e];
    }
    if (ood_out) memcpy(ood_out, ood.data(), 8 * (size_t)n_ood);
    deep_transcript_gammas(tr, ood.data(), W, K, D, &gammas);
    const FsSeed seed = tr.seed();
    deep_compose_build(ctx->fs.F, g, W, D, w_n, z, ood.data(), gammas.data(), &ctab);
    HIP_TRY(ctx, hipMemcpyAsync(d_ctab, ctab.data(), ctab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_compose_enqueue(ctx, W, D, log_N, (uint32_t)cfg->lde_offset, d_ctab, d_lde, N, d_seg, N, d_cw, N));
    mark(5);
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    FriExtResult xres;
    SMI_TRY(fri_run_ext(ctx, &fc, &seed, d_cw, N, N, false, &xres, (int)grind_bits));
    std::vector<uint8_t> bytes(9 + 8 * (size_t)n_ood);
    bytes[0] = 2;
    for (int i = 0; i < 8; i++) bytes[1 + i] = (uint8_t)((uint64_t)n_ood >> (8 * i));
    for (uint32_t v = 0; v < n_ood; v++)
        for (int i = 0; i < 8; i++) bytes[9 + 8 * (size_t)v + i] = (uint8_t)(ood[v] >> (8 * i));
    bytes.insert(bytes.end(), xres.proof.begin(), xres.proof.end());
    if (top_indices) memcpy(top_indices, xres.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    mark(6);
    if (cfg->num_colinearity_tests) {
        const uint32_t t = (uint32_t)cfg->num_colinearity_tests, R = 2;
        const size_t ob1 = (size_t)mg_row_open_bytes(W, t, log_N, R), ob2 = (size_t)mg_row_open_bytes(4 * D, t, log_N, R);
        uint64_t *d_top = (uint64_t *)arena_alloc(ctx, 8 * (size_t)t);
        uint8_t *d_open = (uint8_t *)arena_alloc(ctx, ob1 + ob2);
        if (!d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, "air_prove_deep: row openings");
        HIP_TRY(ctx, hipMemcpyAsync(d_top, xres.top.data(), 8 * (size_t)t, hipMemcpyHostToDevice, ctx->stream));
        SMI_TRY(launch_air_row_open(ctx, d_lde, N, W, tree1, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open));
        SMI_TRY(launch_air_row_open(ctx, d_seg, N, 4 * D, tree2, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open + ob1));
        const size_t at = bytes.size();
        bytes.resize(at + ob1 + ob2);
        HIP_TRY(ctx, hipMemcpyAsync(bytes.data() + at, d_open, ob1 + ob2, hipMemcpyDeviceToHost, ctx->stream));
    }
    mark(7);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (timed)
        for (int i = 0; i < 7; i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1]);
            stage_ms[i] = ms;
        }
    return smi_proof_out(ctx, bytes, proof, proof_len);
}

// ---- out-of-domain sampling with an argument list (include/stark_mi.h, "Out-of-domain sampling with an argument list")
// deep_compose_kernel with the 4 A extended coordinate columns of the auxiliary F_q columns as a third group of streams:
// 4 (W + 4 A + 4 D) + 16 bytes a point, one 16-byte load per column and lane.  The lane body (deep_core.h) keeps one column
// group live at a time, so the register count does not grow with A; the gammas are scalar loads of the table.
template <bool VEC>
__global__ __launch_bounds__(DEEP_BLOCK) void deep_compose_args_kernel(Fp F, uint32_t g_m, uint32_t W, uint32_t A, uint32_t D, uint64_t N, uint32_t h_m,
                                                                        uint32_t omega_m, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ lde,
                                                                        size_t stride, const uint32_t *__restrict__ cl, size_t c_stride,
                                                                        const uint32_t *__restrict__ seg, size_t seg_stride, uint32_t *__restrict__ out,
                                                                        size_t out_stride) {
    const uint64_t groups = N / DEEP_ROWS, gid = (uint64_t)blockIdx.x * DEEP_BLOCK + threadIdx.x, gstep = (uint64_t)gridDim.x * DEEP_BLOCK;
    uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * DEEP_ROWS, F), F);
    const uint32_t xstep_m = mont_pow(omega_m, gstep * DEEP_ROWS, F);
    for (uint64_t g = gid; g < groups; g += gstep) {
        const uint64_t i0 = g * DEEP_ROWS;   // N is a multiple of 4: i0 + 3 < N
        uint32_t o[4][DEEP_ROWS];
        deep_compose_args_points(
            tab, W, A, D, g_m, F, x_m, omega_m, [&](uint32_t c, uint32_t v[4]) { perm_load4<VEC>(lde + (size_t)c * stride, i0, N, v); },
            [&](uint32_t col, uint32_t v[4]) { perm_load4<VEC>(cl + (size_t)col * c_stride, i0, N, v); },
            [&](uint32_t col, uint32_t v[4]) { perm_load4<VEC>(seg + (size_t)col * seg_stride, i0, N, v); }, o);
#pragma unroll
        for (int e = 0; e < 4; e++) perm_store4<VEC>(out + e * out_stride, i0, N, o[e]);
        x_m = mont_mul(x_m, xstep_m, F);
    }
}

namespace {
// d_tab: the table of deep_compose_args_build on the device
int deep_compose_args_enqueue(smi_ctx *ctx, uint32_t W, uint32_t A, uint32_t D, uint32_t log_N, uint32_t h, const uint32_t *d_tab, const uint32_t *d_lde,
                              size_t stride, const uint32_t *d_cl, size_t c_stride, const uint32_t *d_seg, size_t seg_stride, uint32_t *d_out,
                              size_t out_stride) {
    const Fp F = ctx->fs.F;
    const uint64_t N = 1ull << log_N;
    const bool vec = al16(d_lde) && al16(d_cl) && al16(d_seg) && al16(d_out) && !(stride & 3) && !(c_stride & 3) && !(seg_stride & 3) && !(out_stride & 3);
    const uint64_t groups = N / DEEP_ROWS, want = (groups + DEEP_BLOCK - 1) / DEEP_BLOCK, cap = (uint64_t)ctx->num_cus * 8;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint32_t g_m = air_to_m(ctx->fs.g, F.p), h_m = air_to_m(h, F.p), omega_m = air_to_m(h_root(ctx, log_N), F.p);
    ProfScope ps(ctx, "deep_compose_args_kernel", (4.0 * (W + 4.0 * A + 4.0 * D) + 16.0) * (double)N);
    if (vec)
        deep_compose_args_kernel<true><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, W, A, D, N, h_m, omega_m, d_tab, d_lde, stride, d_cl, c_stride, d_seg,
                                                                             seg_stride, d_out, out_stride);
    else
        deep_compose_args_kernel<false><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, W, A, D, N, h_m, omega_m, d_tab, d_lde, stride, d_cl, c_stride, d_seg,
                                                                              seg_stride, d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
}  // namespace

int smi_dev_deep_compose_args(smi_ctx *ctx, const smi_stark_cfg *cfg, uint32_t n_args, uint32_t n_segments, const uint32_t *d_lde, size_t stride,
                              const uint32_t *d_c_lde, size_t c_stride, const uint32_t *d_seg, size_t seg_stride, const uint64_t z[4], const uint64_t *ood,
                              const uint64_t *challenges, uint32_t *d_out, size_t out_stride) {
    if (!ctx || !cfg || !d_lde || !d_c_lde || !d_seg || !z || !ood || !challenges || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(deep_field_check(ctx));
    const uint32_t W = cfg->n_cols, A = n_args, D = n_segments, log_N = cfg->log_n + cfg->log_blowup;
    if (!W || W > 64) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose_args: 1..64 columns");
    if (!A || A > SMI_ARGS_MAX) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose_args: 1 .. 8 auxiliary columns");
    if (!D || D > DEEP_MAX_SEGMENTS) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose_args: 1 .. 16 segments");
    if (cfg->log_n < 1 || cfg->log_blowup < 2 || log_N > 27)
        return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose_args: log_n >= 1, log_blowup >= 2, log_n + log_blowup <= 27");
    if (log_N > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    const uint64_t N = 1ull << log_N;
    if (stride < N || c_stride < N || seg_stride < N || out_stride < N)
        return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose_args: stride < N, c_stride < N, seg_stride < N or out_stride < N");
    if (!cfg->lde_offset || cfg->lde_offset >= ctx->fs.F.p) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose_args: lde_offset must be in 1 .. p-1");
    FqH zq;
    SMI_TRY(deep_point(ctx, z, &zq));
    if (fqh_in_base(zq)) return smi_fail(ctx, SMI_ERR_BAD_ARG, DEEP_Z_IN_BASE_FIELD);
    for (size_t i = 0; i < deep_args_record(W, A, D); i++)
        if (ood[i] >= ctx->fs.F.p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "deep_compose_args: an out-of-domain coordinate is >= p");
    std::vector<uint32_t> tab;
    deep_compose_args_build(ctx->fs.F, ctx->fs.g, W, A, D, h_root(ctx, cfg->log_n), zq, ood, challenges, &tab);
    void *d_tab = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, tab.size() * 4, &d_tab));
    HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    return deep_compose_args_enqueue(ctx, W, A, D, log_N, (uint32_t)cfg->lde_offset, (const uint32_t *)d_tab, d_lde, stride, d_c_lde, c_stride, d_seg,
                                     seg_stride, d_out, out_stride);
}

int smi_dev_air_prove_deep_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const void *xargs_, const uint32_t *d_trace_cols,
                                 uint8_t *roots_out, uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms,
                                 uint32_t grind_bits, uint32_t *closes) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_xargs *xargs = (const smi_air_xargs *)xargs_;
    if (!ctx || !cfg || !air || !xargs || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(deep_field_check(ctx));
    uint32_t D = 0;
    {
        std::string why;
        const int rc = deep_xargs_plan(ctx->fs.F.p, cfg, air, xargs, nullptr, &D, &why);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    SMI_TRY(xargs_entry_checks(ctx, air, xargs, cfg->n_cols, cfg->log_n));
    const uint32_t W = cfg->n_cols, K = air->n_constraints, A = xargs->count, log_n = cfg->log_n, log_N = cfg->log_n + cfg->log_blowup;
    const uint32_t NW = W + K + 2 * A, CW = 4 * A;   // weights; coordinate columns of the second tree
    if (log_N > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    const size_t n = (size_t)1 << log_n, N = (size_t)1 << log_N;
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, log_n);
    AirHost H;
    air_build(ctx->fs.F, h_root(ctx, log_N), cfg, air, &H);
    SMI_TRY(arena_reset(ctx));
    struct Events {   // destroyed on every return path
        hipEvent_t ev[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } evs;
    const bool timed = stage_ms != nullptr;
    if (timed)
        for (int i = 0; i < 9; i++) HIP_TRY(ctx, hipEventCreate(&evs.ev[i]));
    auto mark = [&](int i) { if (timed) (void)hipEventRecord(evs.ev[i], ctx->stream); };

    const size_t n_ood = deep_args_record(W, A, D);
    const size_t tree_bytes = 2 * N * 32, w_tab1 = deep_eval_tab_words(1), w_tab2 = deep_eval_tab_words(2);
    const size_t part_a = deep_eval_part_bytes(W + CW, n, 2), part_b = deep_eval_part_bytes(D, n, 1);
    uint32_t *d_lde = (uint32_t *)arena_alloc(ctx, (size_t)W * N * 4);
    uint32_t *d_c = (uint32_t *)arena_alloc(ctx, (size_t)CW * n * 4);
    uint32_t *d_cl = (uint32_t *)arena_alloc(ctx, (size_t)CW * N * 4);
    uint32_t *d_cw = (uint32_t *)arena_alloc(ctx, 4 * N * 4);        // H, then Q
    uint32_t *d_hc = (uint32_t *)arena_alloc(ctx, 4 * N * 4);        // the coefficients of H's coordinates
    uint32_t *d_seg = (uint32_t *)arena_alloc(ctx, 4 * (size_t)D * N * 4);
    uint32_t *d_coef = (uint32_t *)arena_alloc(ctx, (size_t)(W + CW) * n * 4);   // the trace polynomials, then the columns' coordinates
    uint64_t *d_weights = (uint64_t *)arena_alloc(ctx, 8 * 4 * (size_t)NW);
    uint32_t *d_blob = (uint32_t *)arena_alloc(ctx, H.blob.size() * 4);
    uint8_t *tree1 = (uint8_t *)arena_alloc(ctx, tree_bytes), *tree2 = (uint8_t *)arena_alloc(ctx, tree_bytes), *tree3 = (uint8_t *)arena_alloc(ctx, tree_bytes);
    uint8_t *d_atmp = (uint8_t *)arena_alloc(ctx, xargs_columns_tmp_size(A, n));
    uint32_t *d_tab2 = (uint32_t *)arena_alloc(ctx, w_tab2 * 4), *d_tab1 = (uint32_t *)arena_alloc(ctx, w_tab1 * 4);
    uint32_t *d_part = (uint32_t *)arena_alloc(ctx, part_a > part_b ? part_a : part_b);
    uint32_t *d_res = (uint32_t *)arena_alloc(ctx, (size_t)(8 * (W + CW) + 16 * D) * 4);   // columns at z and z w | H_{j,e} at z, e-major
    uint32_t *d_ctab = (uint32_t *)arena_alloc(ctx, deep_args_tab_words(W, A, D) * 4);
    uint32_t *d_ptab = nullptr, *d_pvals = nullptr;
    if (H.dev.Q) {
        d_ptab = (uint32_t *)arena_alloc(ctx, H.per.table_words * 4);
        d_pvals = (uint32_t *)arena_alloc(ctx, H.per.vals.size() * 4);
    }
    if (!d_lde || !d_c || !d_cl || !d_cw || !d_hc || !d_seg || !d_coef || !d_weights || !d_blob || !tree1 || !tree2 || !tree3 || !d_atmp || !d_tab2 ||
        !d_tab1 || !d_part || !d_res || !d_ctab || (H.dev.Q && (!d_ptab || !d_pvals)))
        return smi_fail(ctx, SMI_ERR_OOM, "air_prove_deep_xargs: device memory");
    mark(0);
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, W, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_lde));
    mark(1);
    SMI_TRY(launch_merkle_rows(ctx, d_lde, W, N, N, tree1));
    mark(2);
    // first round trip: root_1 -> alpha, gamma
    uint8_t roots[96];
    HIP_TRY(ctx, hipMemcpyAsync(roots, tree1 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, d_pvals, d_ptab));   // queued before the host waits for the root; d_pvals: the raw values the column build reads
    SMI_TRY(dev_ntt(ctx, d_trace_cols, d_coef, log_n, n, W, n, n, 1, cfg->trace_offset, 1));   // the trace polynomials, for step 7
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    Transcript tr;
    std::vector<uint64_t> ch, weights, gammas;   // 8 challenges; 4 NW weights; the record's gammas
    transcript_perm_challenges(tr, roots, &ch);
    XArgsDev XD;
    xargs_build(ctx->fs.F, g, xargs, W, air, H.per, ch.data(), &XD);
    XD.pvals = d_pvals;
    SMI_TRY(xargs_columns_launch(ctx, XD, d_trace_cols, log_n, d_c, n, d_atmp));
    SMI_TRY(smi_dev_lde(ctx, d_c, CW, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_cl));
    SMI_TRY(launch_merkle_rows(ctx, d_cl, CW, N, N, tree2));
    mark(3);
    // second round trip: root_2 (and the columns' verdicts) -> the weights
    ArgsFlags fl;
    HIP_TRY(ctx, hipMemcpyAsync(roots + 32, tree2 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&fl, xargs_columns_flags_at(d_atmp, A, n), sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    SMI_TRY(dev_ntt(ctx, d_c, d_coef + (size_t)W * n, log_n, n, CW, n, n, 1, cfg->trace_offset, 1));   // the columns' coordinates as polynomials
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    SMI_TRY(xargs_columns_settle(ctx, XD, fl, closes));
    transcript_args_weights(tr, roots + 32, W, K, A, &weights);
    HIP_TRY(ctx, hipMemcpyAsync(d_weights, weights.data(), 8 * weights.size(), hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(air_compose_ext_launch(ctx, H, d_blob, d_lde, N, d_weights, d_cw, N));
    SMI_TRY(xargs_compose_launch(ctx, XD, H, (uint32_t)cfg->trace_offset, d_lde, N, d_cl, N, d_weights + 4 * (size_t)(W + K), d_cw, N));
    mark(4);
    // the segments: coefficients of every coordinate of H on the coset, D slices of n, each extended back to the N points
    SMI_TRY(dev_ntt(ctx, d_cw, d_hc, log_N, N, 4, N, N, 1, cfg->lde_offset, 1));
    for (uint32_t j = 0; j < D; j++)
        SMI_TRY(dev_ntt(ctx, d_hc + (size_t)j * n, d_seg + 4 * (size_t)j * N, log_N, n, 4, N, N, 0, cfg->lde_offset, 1));
    SMI_TRY(launch_merkle_rows(ctx, d_seg, 4 * D, N, N, tree3));
    mark(5);
    // third round trip: root_3 -> z
    HIP_TRY(ctx, hipMemcpyAsync(roots + 64, tree3 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t zr[4];
    deep_args_transcript_z(tr, roots + 64, NW, zr);
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return smi_fail(ctx, SMI_ERR_BAD_ARG, DEEP_Z_IN_BASE_FIELD);
    if (roots_out) memcpy(roots_out, roots, 96);
    // fourth round trip: u, v = f(z), f(z w); a, b = c(z), c(z w); s = H_j(z)
    const FqH pts[2] = {z, fqh_scale(z, w_n, p)};
    std::vector<uint32_t> tab2, tab1, ctab, res(8 * (size_t)(W + CW) + 16 * (size_t)D);
    deep_eval_build(ctx->fs.F, g, 2, pts, &tab2);
    deep_eval_build(ctx->fs.F, g, 1, pts, &tab1);
    HIP_TRY(ctx, hipMemcpyAsync(d_tab2, tab2.data(), tab2.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_tab1, tab1.data(), tab1.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_eval_enqueue(ctx, d_coef, W + CW, n, n, 2, d_tab2, d_part, d_res));
    uint32_t *d_sres = d_res + 8 * (size_t)(W + CW);
    for (uint32_t e = 0; e < 4; e++)   // coordinate e of the D segments: D columns of n coefficients, n apart
        SMI_TRY(deep_eval_enqueue(ctx, d_hc + (size_t)e * N, D, n, n, 1, d_tab1, d_part, d_sres + 4 * (size_t)e * D));
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_res, res.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> ood(n_ood);
    const FqH X{{0, 1 % p, 0, 0}};
    auto assemble = [&](const uint32_t *at, size_t pitch, uint64_t *dst) {   // sum_e X^e v_e, v_e four words at at + e pitch
        FqH s = fqh(0), xe = fqh(1 % p);
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t *v = at + e * pitch;
            s = fqh_add(s, fqh_mul(xe, FqH{{v[0], v[1], v[2], v[3]}}, p, g), p);
            xe = fqh_mul(xe, X, p, g);
        }
        for (uint32_t e = 0; e < 4; e++) dst[e] = s.c[e];
    };
    for (uint32_t c = 0; c < W; c++)
        for (uint32_t e = 0; e < 4; e++) ood[4 * c + e] = res[8 * c + e], ood[4 * (W + c) + e] = res[8 * c + 4 + e];
    for (uint32_t a = 0; a < A; a++) {   // coordinate column 4 a + e at z: res[8 (W + 4 a + e) ..], at z w: four words on
        assemble(&res[8 * (size_t)(W + 4 * a)], 8, &ood[4 * (2 * (size_t)W + a)]);
        assemble(&res[8 * (size_t)(W + 4 * a) + 4], 8, &ood[4 * (2 * (size_t)W + A + a)]);
    }
    for (uint32_t j = 0; j < D; j++) assemble(&res[8 * (size_t)(W + CW) + 4 * (size_t)j], 4 * (size_t)D, &ood[4 * (2 * (size_t)W + 2 * (size_t)A + j)]);
    if (ood_out) memcpy(ood_out, ood.data(), 8 * n_ood);
    deep_args_transcript_gammas(tr, ood.data(), NW, n_ood, &gammas);
    const FsSeed seed = tr.seed();
    deep_compose_args_build(ctx->fs.F, g, W, A, D, w_n, z, ood.data(), gammas.data(), &ctab);
    HIP_TRY(ctx, hipMemcpyAsync(d_ctab, ctab.data(), ctab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_compose_args_enqueue(ctx, W, A, D, log_N, (uint32_t)cfg->lde_offset, d_ctab, d_lde, N, d_cl, N, d_seg, N, d_cw, N));
    mark(6);
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    FriExtResult xres;
    SMI_TRY(fri_run_ext(ctx, &fc, &seed, d_cw, N, N, false, &xres, (int)grind_bits));
    std::vector<uint8_t> bytes(9 + 8 * n_ood);
    bytes[0] = 2;
    for (int i = 0; i < 8; i++) bytes[1 + i] = (uint8_t)((uint64_t)n_ood >> (8 * i));
    for (size_t v = 0; v < n_ood; v++)
        for (int i = 0; i < 8; i++) bytes[9 + 8 * v + i] = (uint8_t)(ood[v] >> (8 * i));
    bytes.insert(bytes.end(), xres.proof.begin(), xres.proof.end());
    if (top_indices) memcpy(top_indices, xres.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    mark(7);
    if (cfg->num_colinearity_tests) {
        const uint32_t t = (uint32_t)cfg->num_colinearity_tests, R = 2;
        const size_t ob1 = (size_t)mg_row_open_bytes(W, t, log_N, R), ob2 = (size_t)mg_row_open_bytes(CW, t, log_N, R),
                     ob3 = (size_t)mg_row_open_bytes(4 * D, t, log_N, R);
        uint64_t *d_top = (uint64_t *)arena_alloc(ctx, 8 * (size_t)t);
        uint8_t *d_open = (uint8_t *)arena_alloc(ctx, ob1 + ob2 + ob3);
        if (!d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, "air_prove_deep_xargs: row openings");
        HIP_TRY(ctx, hipMemcpyAsync(d_top, xres.top.data(), 8 * (size_t)t, hipMemcpyHostToDevice, ctx->stream));
        SMI_TRY(launch_air_row_open(ctx, d_lde, N, W, tree1, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open));
        SMI_TRY(launch_air_row_open(ctx, d_cl, N, CW, tree2, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open + ob1));
        SMI_TRY(launch_air_row_open(ctx, d_seg, N, 4 * D, tree3, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open + ob1 + ob2));
        const size_t at = bytes.size();
        bytes.resize(at + ob1 + ob2 + ob3);
        HIP_TRY(ctx, hipMemcpyAsync(bytes.data() + at, d_open, ob1 + ob2 + ob3, hipMemcpyDeviceToHost, ctx->stream));
    }
    mark(8);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (timed)
        for (int i = 0; i < 8; i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1]);
            stage_ms[i] = ms;
        }
    return smi_proof_out(ctx, bytes, proof, proof_len);
}

// ---- out-of-domain sampling over coset leaves (include/stark_mi.h, "Out-of-domain sampling over coset leaves")
// The two provers above with every commitment a tree of coset leaves (launch_merkle_cosets), FRI at folding factor 4 over
// the DEEP codeword where it stands (stride == N: no compaction copy), and one leaf and one path per test and group
// (coset_open_kernel).  Everything else -- the transcripts, the segments, the evaluations at z, the two codeword kernels --
// is what the provers above run, so the two variants are one function that differs by the list (xargs == nullptr: a plain
// AIR) and by the group table.

// one workgroup per (test, group): mgpu_core.h mg_coset_open_write
__global__ __launch_bounds__(64) void coset_open_kernel(const MgCosetTable tab, uint32_t log_N, const uint64_t *__restrict__ top, uint32_t t, uint8_t *out) {
    const MgCosetGroup &G = tab.g[blockIdx.y];
    mg_coset_open_write(G, log_N, top[blockIdx.x], blockIdx.x, t, out + G.out_at, threadIdx.x, 64);
}

namespace {
int deep_fold4_prove(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, const uint32_t *d_trace_cols, uint8_t *roots_out,
                     uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, uint32_t *closes) {
    if (closes) *closes = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(deep_field_check(ctx));
    uint32_t D = 0;
    {
        std::string why;
        const int rc = xargs ? deep_xargs_plan(ctx->fs.F.p, cfg, air, xargs, nullptr, &D, &why) : deep_plan(ctx->fs.F.p, cfg, air, nullptr, &D, &why);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    if (xargs) SMI_TRY(xargs_entry_checks(ctx, air, xargs, cfg->n_cols, cfg->log_n));
    const uint32_t W = cfg->n_cols, K = air->n_constraints, A = xargs ? xargs->count : 0, log_n = cfg->log_n, log_N = cfg->log_n + cfg->log_blowup;
    const uint32_t NW = W + K + 2 * A, CW = 4 * A;   // weights; coordinate columns of the auxiliary tree
    if (log_N > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    if (fri_layout_fold4(deep_fri_cfg(cfg, 1)).F == 0) return smi_fail(ctx, SMI_ERR_BAD_ARG, DEEP_FOLD4_NO_LAYER);
    const size_t n = (size_t)1 << log_n, N = (size_t)1 << log_N, q = N / 4;
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, log_n);
    const uint32_t G = A ? 3 : 2, n_stages = A ? 8 : 7;
    AirHost H;
    air_build(ctx->fs.F, h_root(ctx, log_N), cfg, air, &H);
    SMI_TRY(arena_reset(ctx));
    struct Events {   // destroyed on every return path
        hipEvent_t ev[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } evs;
    const bool timed = stage_ms != nullptr;
    if (timed)
        for (uint32_t i = 0; i <= n_stages; i++) HIP_TRY(ctx, hipEventCreate(&evs.ev[i]));
    uint32_t marks = 0;
    auto mark = [&]() {
        if (timed) (void)hipEventRecord(evs.ev[marks], ctx->stream);
        marks++;
    };

    const size_t n_ood = deep_args_record(W, A, D);
    const size_t tree_bytes = 2 * q * 32, w_tab1 = deep_eval_tab_words(1), w_tab2 = deep_eval_tab_words(2);
    const size_t part_a = deep_eval_part_bytes(W + CW, n, 2), part_b = deep_eval_part_bytes(D, n, 1);
    uint32_t *d_lde = (uint32_t *)arena_alloc(ctx, (size_t)W * N * 4);
    uint32_t *d_c = A ? (uint32_t *)arena_alloc(ctx, (size_t)CW * n * 4) : nullptr;
    uint32_t *d_cl = A ? (uint32_t *)arena_alloc(ctx, (size_t)CW * N * 4) : nullptr;
    uint32_t *d_cw = (uint32_t *)arena_alloc(ctx, 4 * N * 4);        // H, then Q
    uint32_t *d_hc = (uint32_t *)arena_alloc(ctx, 4 * N * 4);        // the coefficients of H's coordinates
    uint32_t *d_seg = (uint32_t *)arena_alloc(ctx, 4 * (size_t)D * N * 4);
    uint32_t *d_coef = (uint32_t *)arena_alloc(ctx, (size_t)(W + CW) * n * 4);   // the trace polynomials, then the columns' coordinates
    uint64_t *d_weights = (uint64_t *)arena_alloc(ctx, 8 * 4 * (size_t)NW);
    uint32_t *d_blob = (uint32_t *)arena_alloc(ctx, H.blob.size() * 4);
    uint8_t *tree[3] = {nullptr, nullptr, nullptr};   // in group order: trace, (auxiliary,) segments
    for (uint32_t k = 0; k < G; k++) tree[k] = (uint8_t *)arena_alloc(ctx, tree_bytes);
    uint8_t *d_atmp = A ? (uint8_t *)arena_alloc(ctx, xargs_columns_tmp_size(A, n)) : nullptr;
    uint32_t *d_tab2 = (uint32_t *)arena_alloc(ctx, w_tab2 * 4), *d_tab1 = (uint32_t *)arena_alloc(ctx, w_tab1 * 4);
    uint32_t *d_part = (uint32_t *)arena_alloc(ctx, part_a > part_b ? part_a : part_b);
    uint32_t *d_res = (uint32_t *)arena_alloc(ctx, (size_t)(8 * (W + CW) + 16 * D) * 4);   // columns at z and z w | H_{j,e} at z, e-major
    uint32_t *d_ctab = (uint32_t *)arena_alloc(ctx, deep_args_tab_words(W, A, D) * 4);
    uint32_t *d_ptab = nullptr, *d_pvals = nullptr;
    if (H.dev.Q) {
        d_ptab = (uint32_t *)arena_alloc(ctx, H.per.table_words * 4);
        d_pvals = (uint32_t *)arena_alloc(ctx, H.per.vals.size() * 4);
    }
    if (!d_lde || (A && (!d_c || !d_cl || !d_atmp)) || !d_cw || !d_hc || !d_seg || !d_coef || !d_weights || !d_blob || !tree[0] || !tree[1] || (A && !tree[2]) ||
        !d_tab2 || !d_tab1 || !d_part || !d_res || !d_ctab || (H.dev.Q && (!d_ptab || !d_pvals)))
        return smi_fail(ctx, SMI_ERR_OOM, "air_prove_deep_fold4: device memory");
    auto root_of = [&](uint32_t k, uint8_t *dst) { return hipMemcpyAsync(dst, tree[k] + (2 * q - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream); };
    mark();
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, W, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_lde));
    mark();
    SMI_TRY(launch_merkle_cosets(ctx, d_lde, W, N, N, tree[0]));
    mark();
    // root_1 -> the composition weights (plain AIR) or alpha, gamma (list)
    uint8_t roots[96];
    HIP_TRY(ctx, root_of(0, roots));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, d_pvals, d_ptab));   // queued before the host waits for the root
    SMI_TRY(dev_ntt(ctx, d_trace_cols, d_coef, log_n, n, W, n, n, 1, cfg->trace_offset, 1));   // the trace polynomials, for the values at z
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    Transcript tr;
    std::vector<uint64_t> ch, weights, gammas;
    XArgsDev XD;
    if (A) {
        transcript_perm_challenges(tr, roots, &ch);
        xargs_build(ctx->fs.F, g, xargs, W, air, H.per, ch.data(), &XD);
        XD.pvals = d_pvals;
        SMI_TRY(xargs_columns_launch(ctx, XD, d_trace_cols, log_n, d_c, n, d_atmp));
        SMI_TRY(smi_dev_lde(ctx, d_c, CW, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_cl));
        SMI_TRY(launch_merkle_cosets(ctx, d_cl, CW, N, N, tree[1]));
        mark();
        // root_2 (and the columns' verdicts) -> the weights
        ArgsFlags fl;
        HIP_TRY(ctx, root_of(1, roots + 32));
        HIP_TRY(ctx, hipMemcpyAsync(&fl, xargs_columns_flags_at(d_atmp, A, n), sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
        SMI_TRY(dev_ntt(ctx, d_c, d_coef + (size_t)W * n, log_n, n, CW, n, n, 1, cfg->trace_offset, 1));   // the columns' coordinates as polynomials
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        SMI_TRY(xargs_columns_settle(ctx, XD, fl, closes));
        transcript_args_weights(tr, roots + 32, W, K, A, &weights);
    } else {
        deep_transcript_weights(tr, roots, W, K, &weights);
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_weights, weights.data(), 8 * weights.size(), hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(air_compose_ext_launch(ctx, H, d_blob, d_lde, N, d_weights, d_cw, N));
    if (A) SMI_TRY(xargs_compose_launch(ctx, XD, H, (uint32_t)cfg->trace_offset, d_lde, N, d_cl, N, d_weights + 4 * (size_t)(W + K), d_cw, N));
    mark();
    // the segments: coefficients of every coordinate of H on the coset, D slices of n, each extended back to the N points
    SMI_TRY(dev_ntt(ctx, d_cw, d_hc, log_N, N, 4, N, N, 1, cfg->lde_offset, 1));
    for (uint32_t j = 0; j < D; j++)
        SMI_TRY(dev_ntt(ctx, d_hc + (size_t)j * n, d_seg + 4 * (size_t)j * N, log_N, n, 4, N, N, 0, cfg->lde_offset, 1));
    SMI_TRY(launch_merkle_cosets(ctx, d_seg, 4 * D, N, N, tree[G - 1]));
    mark();
    // the segments' root -> z
    HIP_TRY(ctx, root_of(G - 1, roots + 32 * (G - 1)));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t zr[4];
    if (A) deep_args_transcript_z(tr, roots + 64, NW, zr);
    else deep_transcript_z(tr, roots + 32, W, K, zr);
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return smi_fail(ctx, SMI_ERR_BAD_ARG, DEEP_Z_IN_BASE_FIELD);
    if (roots_out) memcpy(roots_out, roots, 32 * (size_t)G);
    // u, v = f(z), f(z w); a, b = c(z), c(z w); s = H_j(z)
    const FqH pts[2] = {z, fqh_scale(z, w_n, p)};
    std::vector<uint32_t> tab2, tab1, ctab, res(8 * (size_t)(W + CW) + 16 * (size_t)D);
    deep_eval_build(ctx->fs.F, g, 2, pts, &tab2);
    deep_eval_build(ctx->fs.F, g, 1, pts, &tab1);
    HIP_TRY(ctx, hipMemcpyAsync(d_tab2, tab2.data(), tab2.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_tab1, tab1.data(), tab1.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_eval_enqueue(ctx, d_coef, W + CW, n, n, 2, d_tab2, d_part, d_res));
    uint32_t *d_sres = d_res + 8 * (size_t)(W + CW);
    for (uint32_t e = 0; e < 4; e++)   // coordinate e of the D segments: D columns of n coefficients, n apart
        SMI_TRY(deep_eval_enqueue(ctx, d_hc + (size_t)e * N, D, n, n, 1, d_tab1, d_part, d_sres + 4 * (size_t)e * D));
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_res, res.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> ood(n_ood);
    const FqH X{{0, 1 % p, 0, 0}};
    auto assemble = [&](const uint32_t *at, size_t pitch, uint64_t *dst) {   // sum_e X^e v_e, v_e four words at at + e pitch
        FqH s = fqh(0), xe = fqh(1 % p);
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t *v = at + e * pitch;
            s = fqh_add(s, fqh_mul(xe, FqH{{v[0], v[1], v[2], v[3]}}, p, g), p);
            xe = fqh_mul(xe, X, p, g);
        }
        for (uint32_t e = 0; e < 4; e++) dst[e] = s.c[e];
    };
    for (uint32_t c = 0; c < W; c++)
        for (uint32_t e = 0; e < 4; e++) ood[4 * c + e] = res[8 * c + e], ood[4 * (W + c) + e] = res[8 * c + 4 + e];
    for (uint32_t a = 0; a < A; a++) {   // coordinate column 4 a + e at z: res[8 (W + 4 a + e) ..], at z w: four words on
        assemble(&res[8 * (size_t)(W + 4 * a)], 8, &ood[4 * (2 * (size_t)W + a)]);
        assemble(&res[8 * (size_t)(W + 4 * a) + 4], 8, &ood[4 * (2 * (size_t)W + A + a)]);
    }
    for (uint32_t j = 0; j < D; j++) assemble(&res[8 * (size_t)(W + CW) + 4 * (size_t)j], 4 * (size_t)D, &ood[4 * (2 * (size_t)W + 2 * (size_t)A + j)]);
    if (ood_out) memcpy(ood_out, ood.data(), 8 * n_ood);
    if (A) deep_args_transcript_gammas(tr, ood.data(), NW, n_ood, &gammas);
    else deep_transcript_gammas(tr, ood.data(), W, K, D, &gammas);
    const FsSeed seed = tr.seed();
    if (A) {
        deep_compose_args_build(ctx->fs.F, g, W, A, D, w_n, z, ood.data(), gammas.data(), &ctab);
        HIP_TRY(ctx, hipMemcpyAsync(d_ctab, ctab.data(), ctab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        SMI_TRY(deep_compose_args_enqueue(ctx, W, A, D, log_N, (uint32_t)cfg->lde_offset, d_ctab, d_lde, N, d_cl, N, d_seg, N, d_cw, N));
    } else {
        deep_compose_build(ctx->fs.F, g, W, D, w_n, z, ood.data(), gammas.data(), &ctab);
        HIP_TRY(ctx, hipMemcpyAsync(d_ctab, ctab.data(), ctab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        SMI_TRY(deep_compose_enqueue(ctx, W, D, log_N, (uint32_t)cfg->lde_offset, d_ctab, d_lde, N, d_seg, N, d_cw, N));
    }
    mark();
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    FriExtResult xres;
    SMI_TRY(fri_run_ext_fold4(ctx, &fc, &seed, d_cw, N, N, false, &xres, grind_bits));
    std::vector<uint8_t> bytes(9 + 8 * n_ood);
    bytes[0] = 2;
    for (int i = 0; i < 8; i++) bytes[1 + i] = (uint8_t)((uint64_t)n_ood >> (8 * i));
    for (size_t v = 0; v < n_ood; v++)
        for (int i = 0; i < 8; i++) bytes[9 + 8 * v + i] = (uint8_t)(ood[v] >> (8 * i));
    bytes.insert(bytes.end(), xres.proof.begin(), xres.proof.end());
    if (top_indices) memcpy(top_indices, xres.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    mark();
    if (cfg->num_colinearity_tests) {
        const uint32_t t = (uint32_t)cfg->num_colinearity_tests;
        const DeepGroups gr = deep_groups(W, A, D);
        const uint32_t *cols[3] = {d_lde, A ? d_cl : d_seg, d_seg};
        MgCosetTable tab;
        memset(&tab, 0, sizeof tab);
        size_t total = 0;
        for (uint32_t k = 0; k < G; k++) {
            tab.g[k] = MgCosetGroup{cols[k], N, tree[k], total, gr.V[k], 0};
            total += (size_t)mg_coset_open_bytes(gr.V[k], t, log_N);
        }
        uint64_t *d_top = (uint64_t *)arena_alloc(ctx, 8 * (size_t)t);
        uint8_t *d_open = (uint8_t *)arena_alloc(ctx, total);
        if (!d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, "air_prove_deep_fold4: coset openings");
        HIP_TRY(ctx, hipMemcpyAsync(d_top, xres.top.data(), 8 * (size_t)t, hipMemcpyHostToDevice, ctx->stream));
        coset_open_kernel<<<dim3(t, G), 64, 0, ctx->stream>>>(tab, log_N, d_top, t, d_open);
        HIP_TRY(ctx, hipGetLastError());
        const size_t at = bytes.size();
        bytes.resize(at + total);
        HIP_TRY(ctx, hipMemcpyAsync(bytes.data() + at, d_open, total, hipMemcpyDeviceToHost, ctx->stream));
    }
    mark();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (timed)
        for (uint32_t i = 0; i < n_stages; i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1]);
            stage_ms[i] = ms;
        }
    return smi_proof_out(ctx, bytes, proof, proof_len);
}
}  // namespace

int smi_dev_air_prove_deep_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t *roots_out, uint64_t *ood_out,
                                 uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return deep_fold4_prove(ctx, cfg, (const smi_air *)air, nullptr, d_trace_cols, roots_out, ood_out, proof, proof_len, top_indices, stage_ms, grind_bits,
                            nullptr);
}
int smi_dev_air_prove_deep_xargs_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint32_t *d_trace_cols,
                                       uint8_t *roots_out, uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms,
                                       uint32_t grind_bits, uint32_t *closes) {
    if (!ctx || !cfg || !air || !xargs || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return deep_fold4_prove(ctx, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, d_trace_cols, roots_out, ood_out, proof, proof_len, top_indices,
                            stage_ms, grind_bits, closes);
}

// ---- zero-knowledge DEEP proofs (include/stark_mi.h, "Zero-knowledge DEEP proofs")
// deep_fold4_prove for a plain AIR with the four changes of the section: the last k_t rows of the trace overwritten in place
// and the derived AIR composed in the caller's place; the masked split (zk_segments_kernel) for the slices of n; the mask
// polynomial R extended with the segments and added to the DEEP codeword by zk_mask_add_kernel; one salt column in each tree.
// Every random value comes from smi_dev_random_fill under the caller's seed and one of the ZK_STREAM_* identifiers.
int smi_dev_air_prove_deep_zk(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, uint32_t *d_trace_cols, const uint8_t seed[32], uint8_t *roots_out,
                              uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    const smi_air *air0 = (const smi_air *)air_;
    if (!ctx || !cfg || !air0 || !d_trace_cols || !seed || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(deep_field_check(ctx));
    uint32_t D = 0, Dp = 0, kt = 0, ks = 0;
    {
        std::string why;
        const int rc = zk_plan(ctx->fs.F.p, cfg, air0, nullptr, &Dp, &kt, &ks, &why, &D);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    const uint32_t W = cfg->n_cols, K = air0->n_constraints, log_n = cfg->log_n, log_N = cfg->log_n + cfg->log_blowup;
    if (log_N > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    if (fri_layout_fold4(deep_fri_cfg(cfg, 1)).F == 0) return smi_fail(ctx, SMI_ERR_BAD_ARG, ZK_NO_LAYER);
    const size_t n = (size_t)1 << log_n, N = (size_t)1 << log_N, q = N / 4;
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, log_n);
    const uint32_t V1 = W + 1, V2 = 4 * Dp + 5, n_stages = 9;
    ZkAir Z;
    {
        std::string why;
        const int rc = zk_derive_air(p, w_n, cfg, air0, &Z, &why);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    const smi_air *air = &Z.air;
    AirHost H;
    air_build(ctx->fs.F, h_root(ctx, log_N), cfg, air, &H);
    SMI_TRY(arena_reset(ctx));
    struct Events {   // destroyed on every return path
        hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } evs;
    const bool timed = stage_ms != nullptr;
    if (timed)
        for (uint32_t i = 0; i <= n_stages; i++) HIP_TRY(ctx, hipEventCreate(&evs.ev[i]));
    uint32_t marks = 0;
    auto mark = [&]() {
        if (timed) (void)hipEventRecord(evs.ev[marks], ctx->stream);
        marks++;
    };

    const size_t n_ood = 4 * (2 * (size_t)W + Dp);
    const size_t tree_bytes = 2 * q * 32, w_tab1 = deep_eval_tab_words(1), w_tab2 = deep_eval_tab_words(2);
    const size_t part_a = deep_eval_part_bytes(W, n, 2), part_b = deep_eval_part_bytes(Dp, n, 1);
    uint32_t *d_rows = (uint32_t *)arena_alloc(ctx, (size_t)W * kt * 4);
    uint32_t *d_lde = (uint32_t *)arena_alloc(ctx, (size_t)V1 * N * 4);     // the trace, then the salt column
    uint32_t *d_cw = (uint32_t *)arena_alloc(ctx, 4 * N * 4);               // H, then Q, then Q + R
    uint32_t *d_hc = (uint32_t *)arena_alloc(ctx, 4 * N * 4);               // the coefficients of H's coordinates
    uint32_t *d_rho = (uint32_t *)arena_alloc(ctx, (size_t)4 * Dp * ks * 4);
    uint32_t *d_sc = (uint32_t *)arena_alloc(ctx, (size_t)(V2 - 1) * n * 4);   // n coefficients a column: 4 D' of the segments, 4 of R
    uint32_t *d_seg = (uint32_t *)arena_alloc(ctx, (size_t)V2 * N * 4);     // their extensions, then the salt column
    uint32_t *d_coef = (uint32_t *)arena_alloc(ctx, (size_t)W * n * 4);
    uint64_t *d_weights = (uint64_t *)arena_alloc(ctx, 8 * 4 * (size_t)(W + K));
    uint32_t *d_blob = (uint32_t *)arena_alloc(ctx, H.blob.size() * 4);
    uint8_t *tree[2] = {(uint8_t *)arena_alloc(ctx, tree_bytes), (uint8_t *)arena_alloc(ctx, tree_bytes)};
    uint32_t *d_tab2 = (uint32_t *)arena_alloc(ctx, w_tab2 * 4), *d_tab1 = (uint32_t *)arena_alloc(ctx, w_tab1 * 4);
    uint32_t *d_part = (uint32_t *)arena_alloc(ctx, part_a > part_b ? part_a : part_b);
    uint32_t *d_res = (uint32_t *)arena_alloc(ctx, (size_t)(8 * W + 16 * Dp) * 4);   // columns at z and z w | H~_{j,e} at z, e-major
    uint32_t *d_ctab = (uint32_t *)arena_alloc(ctx, deep_tab_words(W, Dp) * 4);
    uint32_t *d_ptab = (uint32_t *)arena_alloc(ctx, H.per.table_words * 4);
    uint32_t *d_pvals = (uint32_t *)arena_alloc(ctx, H.per.vals.size() * 4);
    if (!d_rows || !d_lde || !d_cw || !d_hc || !d_rho || !d_sc || !d_seg || !d_coef || !d_weights || !d_blob || !tree[0] || !tree[1] || !d_tab2 || !d_tab1 ||
        !d_part || !d_res || !d_ctab || !d_ptab || !d_pvals)
        return smi_fail(ctx, SMI_ERR_OOM, "air_prove_deep_zk: device memory");
    auto root_of = [&](uint32_t k, uint8_t *dst) { return hipMemcpyAsync(dst, tree[k] + (2 * q - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream); };
    mark();
    // the randomisers: column c takes elements c k_t .. (c + 1) k_t - 1 of their stream in its last k_t rows; the two salts
    SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_ROWS, d_rows, (size_t)W * kt));
    HIP_TRY(ctx, hipMemcpy2DAsync(d_trace_cols + (n - kt), n * 4, d_rows, (size_t)kt * 4, (size_t)kt * 4, W, hipMemcpyDeviceToDevice, ctx->stream));
    SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_SALT1, d_lde + (size_t)W * N, N));
    SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_SALT2, d_seg + (size_t)(V2 - 1) * N, N));
    mark();
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, W, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_lde));
    mark();
    SMI_TRY(launch_merkle_cosets(ctx, d_lde, V1, N, N, tree[0]));
    mark();
    // root_1 -> the composition weights
    uint8_t roots[64];
    HIP_TRY(ctx, root_of(0, roots));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, d_pvals, d_ptab));   // queued before the host waits for the root
    SMI_TRY(dev_ntt(ctx, d_trace_cols, d_coef, log_n, n, W, n, n, 1, cfg->trace_offset, 1));   // the trace polynomials, for the values at z
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    Transcript tr;
    std::vector<uint64_t> weights, gammas;
    deep_transcript_weights(tr, roots, W, K, &weights);
    HIP_TRY(ctx, hipMemcpyAsync(d_weights, weights.data(), 8 * weights.size(), hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(air_compose_ext_launch(ctx, H, d_blob, d_lde, N, d_weights, d_cw, N));
    mark();
    // the masked segments and R as coefficients, one batched extension, the second tree
    SMI_TRY(dev_ntt(ctx, d_cw, d_hc, log_N, N, 4, N, N, 1, cfg->lde_offset, 1));
    if (Dp > 1) SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_RHO, d_rho, (size_t)4 * (Dp - 1) * ks));
    SMI_TRY(smi_dev_zk_segments(ctx, d_hc, N, (size_t)D * n, log_n, ks, Dp, d_rho, d_sc, n));
    SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_MASK, d_sc + (size_t)4 * Dp * n, 4 * n));
    for (uint32_t c = 0; c < V2 - 1; c += 4)
        SMI_TRY(dev_ntt(ctx, d_sc + (size_t)c * n, d_seg + (size_t)c * N, log_N, n, 4, n, N, 0, cfg->lde_offset, 1));
    SMI_TRY(launch_merkle_cosets(ctx, d_seg, V2, N, N, tree[1]));
    mark();
    // root_2 -> z
    HIP_TRY(ctx, root_of(1, roots + 32));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t zr[4];
    deep_transcript_z(tr, roots + 32, W, K, zr);
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return smi_fail(ctx, SMI_ERR_BAD_ARG, DEEP_Z_IN_BASE_FIELD);
    if (roots_out) memcpy(roots_out, roots, 64);
    // u, v = f(z), f(z w); s_j = H~_j(z)
    const FqH pts[2] = {z, fqh_scale(z, w_n, p)};
    std::vector<uint32_t> tab2, tab1, ctab, res(8 * (size_t)W + 16 * (size_t)Dp);
    deep_eval_build(ctx->fs.F, g, 2, pts, &tab2);
    deep_eval_build(ctx->fs.F, g, 1, pts, &tab1);
    HIP_TRY(ctx, hipMemcpyAsync(d_tab2, tab2.data(), tab2.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_tab1, tab1.data(), tab1.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_eval_enqueue(ctx, d_coef, W, n, n, 2, d_tab2, d_part, d_res));
    uint32_t *d_sres = d_res + 8 * (size_t)W;
    for (uint32_t e = 0; e < 4; e++)   // coordinate e of the D' segments: D' columns of n coefficients, 4 n apart
        SMI_TRY(deep_eval_enqueue(ctx, d_sc + (size_t)e * n, Dp, n, 4 * n, 1, d_tab1, d_part, d_sres + 4 * (size_t)e * Dp));
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_res, res.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> ood(n_ood);
    const FqH X{{0, 1 % p, 0, 0}};
    for (uint32_t c = 0; c < W; c++)
        for (uint32_t e = 0; e < 4; e++) ood[4 * c + e] = res[8 * c + e], ood[4 * (W + c) + e] = res[8 * c + 4 + e];
    for (uint32_t j = 0; j < Dp; j++) {   // s_j = sum_e X^e H~_{j,e}(z)
        FqH s = fqh(0), xe = fqh(1 % p);
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t *v = &res[8 * (size_t)W + 4 * ((size_t)e * Dp + j)];
            s = fqh_add(s, fqh_mul(xe, FqH{{v[0], v[1], v[2], v[3]}}, p, g), p);
            xe = fqh_mul(xe, X, p, g);
        }
        for (uint32_t e = 0; e < 4; e++) ood[4 * (2 * (size_t)W + j) + e] = s.c[e];
    }
    if (ood_out) memcpy(ood_out, ood.data(), 8 * n_ood);
    deep_transcript_gammas(tr, ood.data(), W, K, Dp, &gammas);
    const FsSeed fseed = tr.seed();
    deep_compose_build(ctx->fs.F, g, W, Dp, w_n, z, ood.data(), gammas.data(), &ctab);
    HIP_TRY(ctx, hipMemcpyAsync(d_ctab, ctab.data(), ctab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_compose_enqueue(ctx, W, Dp, log_N, (uint32_t)cfg->lde_offset, d_ctab, d_lde, N, d_seg, N, d_cw, N));
    mark();
    SMI_TRY(zk_mask_add_launch(ctx, d_cw, N, d_seg + (size_t)4 * Dp * N, N, N));   // Q' = Q + R
    mark();
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    FriExtResult xres;
    SMI_TRY(fri_run_ext_fold4(ctx, &fc, &fseed, d_cw, N, N, false, &xres, grind_bits));
    std::vector<uint8_t> bytes(9 + 8 * n_ood);
    bytes[0] = 2;
    for (int i = 0; i < 8; i++) bytes[1 + i] = (uint8_t)((uint64_t)n_ood >> (8 * i));
    for (size_t v = 0; v < n_ood; v++)
        for (int i = 0; i < 8; i++) bytes[9 + 8 * v + i] = (uint8_t)(ood[v] >> (8 * i));
    bytes.insert(bytes.end(), xres.proof.begin(), xres.proof.end());
    if (top_indices) memcpy(top_indices, xres.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    mark();
    if (cfg->num_colinearity_tests) {
        const uint32_t t = (uint32_t)cfg->num_colinearity_tests;
        MgCosetTable tab;
        memset(&tab, 0, sizeof tab);
        const size_t ob1 = (size_t)mg_coset_open_bytes(V1, t, log_N), total = ob1 + (size_t)mg_coset_open_bytes(V2, t, log_N);
        tab.g[0] = MgCosetGroup{d_lde, N, tree[0], 0, V1, 0};
        tab.g[1] = MgCosetGroup{d_seg, N, tree[1], ob1, V2, 0};
        uint64_t *d_top = (uint64_t *)arena_alloc(ctx, 8 * (size_t)t);
        uint8_t *d_open = (uint8_t *)arena_alloc(ctx, total);
        if (!d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, "air_prove_deep_zk: coset openings");
        HIP_TRY(ctx, hipMemcpyAsync(d_top, xres.top.data(), 8 * (size_t)t, hipMemcpyHostToDevice, ctx->stream));
        coset_open_kernel<<<dim3(t, 2), 64, 0, ctx->stream>>>(tab, log_N, d_top, t, d_open);
        HIP_TRY(ctx, hipGetLastError());
        const size_t at = bytes.size();
        bytes.resize(at + total);
        HIP_TRY(ctx, hipMemcpyAsync(bytes.data() + at, d_open, total, hipMemcpyDeviceToHost, ctx->stream));
    }
    mark();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (timed)
        for (uint32_t i = 0; i < n_stages; i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1]);
            stage_ms[i] = ms;
        }
    return smi_proof_out(ctx, bytes, proof, proof_len);
}
