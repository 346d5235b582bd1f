// deep.hip -- out-of-domain sampling (include/stark_mi.h, "Out-of-domain sampling"): coefficient columns evaluated at one or
// two points of F_q, the DEEP codeword (plain and with an argument list), and the provers.  The lane bodies and the host
// tables are deep_core.h, shared with the CPU emulator (emu_deep.cpp); the verifier is in verify.hip.
//
// The provers -- row or coset leaves, plain or with a list, zero-knowledge -- are one set of step functions over a
// DeepProver (shapes, buffers, transcript, record, proof bytes, stage timer) and two short drivers, deep_prove and zk_prove,
// at the end of the file; the six public entry points check their pointers and call a driver.
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
//
// Transition windows (include/stark_mi.h, "AIR: transition windows").  A window of S = 3 or 4 rows opens the trace at
// z w^s, s < S.  The evaluation takes a table per point: deep_eval_kernel<VEC, 3> and <VEC, 4> hold 16 S powers a lane and
// keep the four multiplies per coefficient and point.  The price is registers: 100 .. 104 VGPRs at three points and
// 132 .. 136 at four, 4 and 3 waves a SIMD against 7 at two points (profiles/air_window_kernel_resources.log).  The other
// route -- one table of powers of z and a multiply by w^(s k) per coefficient and shift -- holds 16 + 4 (S - 1) words a
// lane but does 4 S + S - 1 multiplies a coefficient, 19 against 16 at S = 4.  The kernel reads four bytes per 16 S
// multiply-reduce chains, all independent of each other, so it is bound by the multiplier and not by latency that more
// waves would hide; it runs over W n coefficients once a proof.  No timing of either route has been taken on a card.
// deep_compose_window_kernel<VEC, S> is deep_compose_kernel with S accumulators a point and the 4 S denominators of a lane
// under one F_q inversion (deep_core.h deep_compose_window_points): 16 S accumulator words and 16 S words of prefix products
// are live together at the inversion, 163 .. 166 VGPRs (3 waves, as deep_compose_kernel) at S = 3 and 208 .. 243 (2 waves)
// at S = 4, no scratch.
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
#include "zkargs_core.h"

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

// deep_compose_kernel for a window of S = 3 or 4 rows: the same stream, S quotient groups
template <bool VEC, int S>
__global__ __launch_bounds__(DEEP_BLOCK) void deep_compose_window_kernel(Fp F, uint32_t g_m, uint32_t W, uint32_t D, uint64_t N, uint32_t h_m, uint32_t omega_m,
                                                                          const uint32_t *__restrict__ tab, const uint32_t *__restrict__ lde, size_t stride,
                                                                          const uint32_t *__restrict__ seg, size_t seg_stride, uint32_t *__restrict__ out,
                                                                          size_t out_stride) {
    const uint64_t groups = N / DEEP_ROWS, gid = (uint64_t)blockIdx.x * DEEP_BLOCK + threadIdx.x, gstep = (uint64_t)gridDim.x * DEEP_BLOCK;
    uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * DEEP_ROWS, F), F);
    const uint32_t xstep_m = mont_pow(omega_m, gstep * DEEP_ROWS, F);
    for (uint64_t g = gid; g < groups; g += gstep) {
        const uint64_t i0 = g * DEEP_ROWS;   // N is a multiple of 4: i0 + 3 < N
        uint32_t o[4][DEEP_ROWS];
        deep_compose_window_points<S>(
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
        if (P == 4) {
            if (vec) deep_eval_kernel<true, 4><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, d_cols, stride, n_cols, n_coeffs, d_tab, d_part);
            else deep_eval_kernel<false, 4><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, d_cols, stride, n_cols, n_coeffs, d_tab, d_part);
        } else if (P == 3) {
            if (vec) deep_eval_kernel<true, 3><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, d_cols, stride, n_cols, n_coeffs, d_tab, d_part);
            else deep_eval_kernel<false, 3><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, d_cols, stride, n_cols, n_coeffs, d_tab, d_part);
        } else if (P == 2) {
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
        if (P == 4) deep_eval_combine_kernel<4><<<dim3(n_cols, 4), DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, d_part, (uint32_t)nb, d_tab, d_out);
        else if (P == 3) deep_eval_combine_kernel<3><<<dim3(n_cols, 3), DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, d_part, (uint32_t)nb, d_tab, d_out);
        else if (P == 2) deep_eval_combine_kernel<2><<<dim3(n_cols, 2), DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, d_part, (uint32_t)nb, d_tab, d_out);
        else deep_eval_combine_kernel<1><<<dim3(n_cols, 1), DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, d_part, (uint32_t)nb, d_tab, d_out);
        HIP_TRY(ctx, hipGetLastError());
    }
    return SMI_OK;
}

// d_tab: the table of deep_compose_build on the device (built for the window S)
int deep_compose_enqueue(smi_ctx *ctx, uint32_t W, uint32_t D, uint32_t log_N, uint32_t h, const uint32_t *d_tab, const uint32_t *d_lde, size_t stride,
                         const uint32_t *d_seg, size_t seg_stride, uint32_t *d_out, size_t out_stride, uint32_t S = 2) {
    const Fp F = ctx->fs.F;
    const uint64_t N = 1ull << log_N;
    const bool vec = al16(d_lde) && al16(d_seg) && al16(d_out) && !(stride & 3) && !(seg_stride & 3) && !(out_stride & 3);
    const uint64_t groups = N / DEEP_ROWS, want = (groups + DEEP_BLOCK - 1) / DEEP_BLOCK, cap = (uint64_t)ctx->num_cus * 8;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint32_t g_m = air_to_m(ctx->fs.g, F.p), h_m = air_to_m(h, F.p), omega_m = air_to_m(h_root(ctx, log_N), F.p);
    ProfScope ps(ctx, S > 2 ? "deep_compose_window_kernel" : "deep_compose_kernel", (4.0 * (W + 4.0 * D) + 16.0) * (double)N);
#define DEEP_WINDOW_LAUNCH(V, S_) \
    deep_compose_window_kernel<V, S_><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, W, D, N, h_m, omega_m, d_tab, d_lde, stride, d_seg, seg_stride, d_out, out_stride)
    if (S == 4) {
        if (vec) DEEP_WINDOW_LAUNCH(true, 4);
        else DEEP_WINDOW_LAUNCH(false, 4);
    } else if (S == 3) {
        if (vec) DEEP_WINDOW_LAUNCH(true, 3);
        else DEEP_WINDOW_LAUNCH(false, 3);
    } else if (vec) deep_compose_kernel<true><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, W, D, N, h_m, omega_m, d_tab, d_lde, stride, d_seg, seg_stride, d_out, out_stride);
    else deep_compose_kernel<false><<<grid, DEEP_BLOCK, 0, ctx->stream>>>(F, g_m, W, D, N, h_m, omega_m, d_tab, d_lde, stride, d_seg, seg_stride, d_out, out_stride);
#undef DEEP_WINDOW_LAUNCH
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

// the points z, z w, .. z w^(n_shifts - 1) through the launches above, a table per point
int smi_dev_poly_eval_ext_shifts(smi_ctx *ctx, const uint32_t *d_coeffs, uint32_t n_cols, size_t n_coeffs, size_t stride, const uint64_t z[4], uint64_t w,
                                 uint32_t n_shifts, uint64_t *out) {
    if (!ctx || !d_coeffs || !z || !out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(deep_field_check(ctx));
    if (!n_cols || n_cols > 65535) return smi_fail(ctx, SMI_ERR_BAD_ARG, "poly_eval_ext_shifts: 1 .. 65535 columns");
    if (!n_coeffs || n_coeffs > ((size_t)1 << 27)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "poly_eval_ext_shifts: 1 .. 2^27 coefficients");
    if (stride < n_coeffs) return smi_fail(ctx, SMI_ERR_BAD_ARG, "poly_eval_ext_shifts: stride < n_coeffs");
    if (n_shifts < 1 || n_shifts > DEEP_MAX_SHIFTS) return smi_fail(ctx, SMI_ERR_BAD_ARG, "poly_eval_ext_shifts: 1 .. SMI_AIR_MAX_WINDOW shifts");
    if (w >= ctx->fs.F.p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "poly_eval_ext_shifts: w is >= p");
    FqH pts[DEEP_MAX_SHIFTS];
    SMI_TRY(deep_point(ctx, z, &pts[0]));
    for (uint32_t k = 1; k < n_shifts; k++) pts[k] = fqh_scale(pts[k - 1], (uint32_t)w, ctx->fs.F.p);
    std::vector<uint32_t> tab;
    deep_eval_build(ctx->fs.F, ctx->fs.g, n_shifts, pts, &tab);
    const size_t b_tab = up16(tab.size() * 4), b_part = up16(deep_eval_part_bytes(n_cols, n_coeffs, n_shifts)), n_out = (size_t)n_cols * n_shifts * 4;
    void *base = nullptr;   // table | partial sums | results
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_part + n_out * 4, &base));
    uint32_t *d_tab = (uint32_t *)base, *d_part = (uint32_t *)((uint8_t *)base + b_tab), *d_out = (uint32_t *)((uint8_t *)base + b_tab + b_part);
    HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_eval_enqueue(ctx, d_coeffs, n_cols, n_coeffs, stride, n_shifts, d_tab, d_part, d_out));
    std::vector<uint32_t> res(n_out);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_out, n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n_out; i++) out[i] = res[i];
    return SMI_OK;
}

int smi_dev_deep_compose(smi_ctx *ctx, const smi_stark_cfg *cfg, uint32_t n_segments, const uint32_t *d_lde, size_t stride, const uint32_t *d_seg,
                         size_t seg_stride, const uint64_t z[4], const uint64_t *ood, const uint64_t *challenges, uint32_t *d_out, size_t out_stride) {
    return smi_dev_deep_compose_window(ctx, cfg, 2, n_segments, d_lde, stride, d_seg, seg_stride, z, ood, challenges, d_out, out_stride);
}

// window = 2: deep_compose_kernel over the same table, word for word what smi_dev_deep_compose launched before the window
int smi_dev_deep_compose_window(smi_ctx *ctx, const smi_stark_cfg *cfg, uint32_t window, uint32_t n_segments, const uint32_t *d_lde, size_t stride,
                                const uint32_t *d_seg, size_t seg_stride, const uint64_t z[4], const uint64_t *ood, const uint64_t *challenges, uint32_t *d_out,
                                size_t out_stride) {
    if (!ctx || !cfg || !d_lde || !d_seg || !z || !ood || !challenges || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(deep_field_check(ctx));
    const uint32_t S = window;
    if (S < 2 || S > SMI_AIR_MAX_WINDOW) return smi_fail(ctx, SMI_ERR_BAD_ARG, "deep_compose_window: window must be in 2 .. SMI_AIR_MAX_WINDOW");
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
    for (size_t i = 0; i < 4 * ((size_t)S * W + D); i++)
        if (ood[i] >= ctx->fs.F.p) return smi_fail(ctx, SMI_ERR_NON_CANONICAL, "deep_compose: an out-of-domain coordinate is >= p");
    std::vector<uint32_t> tab;
    deep_compose_build(ctx->fs.F, ctx->fs.g, W, D, h_root(ctx, cfg->log_n), zq, ood, challenges, &tab, S);
    void *d_tab = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, tab.size() * 4, &d_tab));
    HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    return deep_compose_enqueue(ctx, W, D, log_N, (uint32_t)cfg->lde_offset, (const uint32_t *)d_tab, d_lde, stride, d_seg, seg_stride, d_out, out_stride, S);
}

// ---- the codeword with an argument list (include/stark_mi.h, "Out-of-domain sampling with an argument list")
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

// ---- the provers (include/stark_mi.h: "Out-of-domain sampling", "... with an argument list", "... over coset leaves",
// "Zero-knowledge DEEP proofs")
// Every variant is a sequence of the steps below over one DeepProver; each step exists once.  deep_prove is the driver of
// {row leaves + FRI at folding factor 2, coset leaves + folding factor 4} x {plain AIR, argument list}: the leaf type
// decides the commit, the FRI call and the openings (DeepProver::cosets), the list adds its columns between root_1 and the
// composition and switches transcript and codeword kernel (DeepProver::A).  zk_prove is the coset-leaf plain driver with the
// steps of its own in between: the randomiser rows and salts before the trace is extended, the masked split in place of the
// slice loop, the mask added to the codeword; its widths V carry the salt columns and R.  The stage marks stand in the
// drivers (and one in deep_list_columns), so a driver reads against the stage_ms list of its section in the header.

// one workgroup per (test, group): mgpu_core.h mg_coset_open_write
__global__ __launch_bounds__(64) void coset_open_kernel(const MgCosetTable tab, uint32_t log_N, const uint64_t *__restrict__ top, uint32_t t, uint8_t *out) {
    const MgCosetGroup &G = tab.g[blockIdx.y];
    mg_coset_open_write(G, log_N, top[blockIdx.x], blockIdx.x, t, out + G.out_at, threadIdx.x, 64);
}

namespace {
struct DeepProver {
    smi_ctx *ctx;
    const smi_stark_cfg *cfg = nullptr;
    const smi_air *air = nullptr;            // what is composed (zk: the derived AIR, once the entry checks are through)
    const smi_air_xargs *xargs = nullptr;    // nullptr: a plain AIR
    const char *name = nullptr;              // the entry point, for the out-of-memory sentences
    bool cosets = false;                     // coset leaves, FRI at folding factor 4; else row leaves, folding factor 2
    const uint32_t *d_trace = nullptr;
    // a zero-knowledge proof with a list: k_t (else 0), the caller's seed, 4 A (k_t - 1) words for the tails of the auxiliary columns
    uint32_t zk_kt = 0;
    const uint8_t *zk_seed = nullptr;
    uint32_t *d_tail = nullptr;
    // shapes (deep_shapes)
    uint32_t W = 0, K = 0, A = 0, CW = 0, NW = 0, D = 0, log_n = 0, log_N = 0, p = 0, g = 0, w_n = 0;   // CW = 4 A coordinate columns; NW weights; D committed segments
    uint32_t S = 2;   // the transition window: the trace is opened at z w^s, s < S (a list or a derived AIR: always 2)
    size_t n = 0, N = 0, leaves = 0, n_ood = 0;
    uint32_t G = 0, V[3] = {0, 0, 0};   // the committed groups in order -- trace, (auxiliary,) segments -- and their widths in columns
    // device buffers (deep_setup); cols[k] and tree[k] are group k's
    uint32_t *d_lde = nullptr, *d_c = nullptr, *d_cl = nullptr, *d_cw = nullptr, *d_hc = nullptr, *d_seg = nullptr, *d_coef = nullptr, *d_blob = nullptr;
    uint32_t *d_tab2 = nullptr, *d_tab1 = nullptr, *d_part = nullptr, *d_res = nullptr, *d_ctab = nullptr, *d_ptab = nullptr, *d_pvals = nullptr;
    uint64_t *d_weights = nullptr;
    uint8_t *d_atmp = nullptr, *tree[3] = {nullptr, nullptr, nullptr};
    const uint32_t *cols[3] = {nullptr, nullptr, nullptr};
    // host state; the vectors that a queued copy reads or fills live as long as the prover
    AirHost H;
    XArgsDev XD;
    XSharedDev SHs;
    const XSharedDev *SH = nullptr;   // &SHs when the list has a shared lookup
    Transcript tr;
    uint8_t roots[96];
    FqH z;
    FsSeed seed;
    std::vector<uint64_t> weights, ood;
    std::vector<uint32_t> ctab;
    FriExtResult fri;
    std::vector<uint8_t> bytes;
    StageTimer timer;
    DeepProver(smi_ctx *c, uint32_t stages, bool timed) : ctx(c), timer(c, stages, timed) {}
};

// the entry checks that follow the variant's plan, in their order, and the shapes; D: the plan's committed segments;
// no_layer: the refusal sentence of a coset variant whose FRI part has no fold
int deep_shapes(DeepProver &s, uint32_t D, const char *no_layer) {
    smi_ctx *ctx = s.ctx;
    const smi_stark_cfg *cfg = s.cfg;
    if (s.xargs) SMI_TRY(xargs_args(ctx, s.air, s.xargs, cfg->n_cols, cfg->log_n));
    s.W = cfg->n_cols, s.K = s.air->n_constraints, s.A = s.xargs ? s.xargs->count : 0, s.D = D, s.log_n = cfg->log_n, s.log_N = cfg->log_n + cfg->log_blowup;
    s.NW = s.W + s.K + 2 * s.A, s.CW = 4 * s.A;
    if (s.log_N > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    if (s.cosets && fri_layout_fold4(deep_fri_cfg(cfg, 1)).F == 0) return smi_fail(ctx, SMI_ERR_BAD_ARG, no_layer);
    s.n = (size_t)1 << s.log_n, s.N = (size_t)1 << s.log_N, s.leaves = s.cosets ? s.N / 4 : s.N;
    s.p = ctx->fs.F.p, s.g = ctx->fs.g, s.w_n = h_root(ctx, s.log_n);
    s.S = s.xargs ? 2 : air_window(s.air);
    s.n_ood = deep_args_record(s.W, s.A, D) + 4 * (size_t)(s.S - 2) * s.W;   // 4 (S W + 2 A + D)
    const DeepGroups gr = deep_groups(s.W, s.A, D);
    s.G = gr.G;
    for (uint32_t k = 0; k < 3; k++) s.V[k] = gr.V[k];
    return SMI_OK;
}

// the AIR's tables, the arena, the timer's events and every buffer the shared steps use, by the variant's widths
int deep_setup(DeepProver &s) {
    smi_ctx *ctx = s.ctx;
    const uint32_t W = s.W, A = s.A, CW = s.CW, D = s.D;
    const size_t n = s.n, N = s.N;
    air_build(ctx->fs.F, h_root(ctx, s.log_N), s.cfg, s.air, &s.H);
    SMI_TRY(arena_reset(ctx));
    HIP_TRY(ctx, s.timer.create());
    bool ok = true;
    auto take = [&](size_t bytes) {
        void *q = arena_alloc(ctx, bytes);
        ok = ok && q;
        return q;
    };
    const size_t part_a = deep_eval_part_bytes(W + CW, n, s.S), part_b = deep_eval_part_bytes(D, n, 1);
    const size_t ctab_a = deep_args_tab_words(W, A, D), ctab_w = deep_window_tab_words(W, D, s.S);
    s.d_lde = (uint32_t *)take((size_t)s.V[0] * N * 4);
    if (A) s.d_c = (uint32_t *)take((size_t)CW * n * 4), s.d_cl = (uint32_t *)take((size_t)s.V[1] * N * 4);   // V[1]: CW, and a salt column under zk
    s.d_cw = (uint32_t *)take(4 * N * 4);   // H, then Q
    s.d_hc = (uint32_t *)take(4 * N * 4);   // the coefficients of H's coordinates
    s.d_seg = (uint32_t *)take((size_t)s.V[s.G - 1] * N * 4);
    s.d_coef = (uint32_t *)take((size_t)(W + CW) * n * 4);   // the trace polynomials, then the columns' coordinates
    s.d_weights = (uint64_t *)take(8 * 4 * (size_t)s.NW);
    s.d_blob = (uint32_t *)take(s.H.blob.size() * 4);
    for (uint32_t k = 0; k < s.G; k++) s.tree[k] = (uint8_t *)take(2 * s.leaves * 32);
    if (A) s.d_atmp = (uint8_t *)take(xargs_columns_tmp_bytes(A, n));
    s.d_tab2 = (uint32_t *)take(deep_eval_tab_words(s.S) * 4), s.d_tab1 = (uint32_t *)take(deep_eval_tab_words(1) * 4);
    s.d_part = (uint32_t *)take(part_a > part_b ? part_a : part_b);
    s.d_res = (uint32_t *)take((size_t)(4 * s.S * (W + CW) + 16 * D) * 4);   // columns at the S points z w^s | the segments' coordinates at z, e-major
    s.d_ctab = (uint32_t *)take((ctab_a > ctab_w ? ctab_a : ctab_w) * 4);
    if (s.H.dev.Q) s.d_ptab = (uint32_t *)take(s.H.per.table_words * 4), s.d_pvals = (uint32_t *)take(s.H.per.vals.size() * 4);
    if (!ok) return smi_fail(ctx, SMI_ERR_OOM, (std::string(s.name) + ": device memory").c_str());
    s.cols[0] = s.d_lde, s.cols[1] = A ? s.d_cl : s.d_seg, s.cols[2] = s.d_seg;
    return SMI_OK;
}

// group k's V[k] columns -> tree[k]: 2 N digests over row leaves, 2 (N / 4) over coset leaves; deep_root_read queues the
// copy of its root to roots + 32 k (a stage mark may stand between the two)
int deep_commit(DeepProver &s, uint32_t k) {
    return s.cosets ? launch_merkle_cosets(s.ctx, s.cols[k], s.V[k], s.N, s.N, s.tree[k]) : launch_merkle_rows(s.ctx, s.cols[k], s.V[k], s.N, s.N, s.tree[k]);
}
hipError_t deep_root_read(DeepProver &s, uint32_t k) {
    return hipMemcpyAsync(s.roots + 32 * k, s.tree[k] + (2 * s.leaves - 2) * 32, 32, hipMemcpyDeviceToHost, s.ctx->stream);
}

// the round trip of root_1; the periodic tables and the trace polynomials (for the values at z) are queued before the host waits
int deep_root1(DeepProver &s) {
    smi_ctx *ctx = s.ctx;
    HIP_TRY(ctx, deep_root_read(s, 0));
    SMI_TRY(air_periodic_tables(ctx, s.cfg, s.H, s.d_pvals, s.d_ptab));
    SMI_TRY(dev_ntt(ctx, s.d_trace, s.d_coef, s.log_n, s.n, s.W, s.n, s.n, 1, s.cfg->trace_offset, 1));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SMI_OK;
}

// a list: root_1 -> alpha, gamma -> the auxiliary columns, extended and committed (a stage of their own); root_2 and the
// columns' verdicts -> the NW weights.  Under zk the tail step follows the column build -- the closing values c_a[n_a] take the
// totals' place in the flags, the rows behind them become random -- and tree 2 gets its salt column.
int deep_list_columns(DeepProver &s, uint32_t *closes) {
    smi_ctx *ctx = s.ctx;
    const smi_stark_cfg *cfg = s.cfg;
    std::vector<uint64_t> ch;   // 8 challenges
    transcript_perm_challenges(s.tr, s.roots, &ch);
    xargs_build(ctx->fs.F, s.g, s.xargs, s.W, s.air, s.H.per, ch.data(), &s.XD);
    s.XD.pvals = s.d_pvals;   // the raw periodic values the column build reads
    s.SH = xshared_build(s.xargs, s.W, &s.SHs) ? &s.SHs : nullptr;
    SMI_TRY(xargs_columns_enqueue(ctx, s.XD, s.SH, s.d_trace, s.log_n, s.d_c, s.n, s.d_atmp));
    if (s.zk_kt) {
        ArgsFlags *d_fl = const_cast<ArgsFlags *>(xargs_columns_flags(s.d_atmp, s.A, s.n));
        SMI_TRY(smi_dev_random_fill(ctx, s.zk_seed, ZK_STREAM_ARGS_TAIL, s.d_tail, (size_t)s.CW * (s.zk_kt - 1)));
        SMI_TRY(zk_args_tail_launch(ctx, s.d_c, s.n, s.log_n, s.zk_kt, s.A, s.d_tail, &d_fl->total[0][0]));
        SMI_TRY(smi_dev_random_fill(ctx, s.zk_seed, ZK_STREAM_SALT_ARGS, s.d_cl + (size_t)s.CW * s.N, s.N));
    }
    SMI_TRY(smi_dev_lde(ctx, s.d_c, s.CW, s.log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, s.d_cl));
    SMI_TRY(deep_commit(s, 1));
    s.timer.mark();
    ArgsFlags fl;
    HIP_TRY(ctx, deep_root_read(s, 1));
    HIP_TRY(ctx, hipMemcpyAsync(&fl, xargs_columns_flags(s.d_atmp, s.A, s.n), sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    SMI_TRY(dev_ntt(ctx, s.d_c, s.d_coef + (size_t)s.W * s.n, s.log_n, s.n, s.CW, s.n, s.n, 1, cfg->trace_offset, 1));   // the columns' coordinates as polynomials
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    SMI_TRY(xargs_columns_verdict(ctx, s.XD, s.SH, fl, closes));
    transcript_indexed(s.tr, s.roots + 32, 8, 4 * (uint64_t)s.NW, &s.weights);   // root_2, then the indices 8 .. 8 + 4 NW - 1
    return SMI_OK;
}

// H on the N points into d_cw: the AIR's quotients under s.weights, plus the list's 2 A auxiliary quotients (3 A under zk)
int deep_compose_h(DeepProver &s) {
    smi_ctx *ctx = s.ctx;
    const size_t N = s.N;
    HIP_TRY(ctx, hipMemcpyAsync(s.d_weights, s.weights.data(), 8 * s.weights.size(), hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(air_compose_ext_launch(ctx, s.H, s.d_blob, s.d_lde, N, s.d_weights, s.d_cw, N));
    const uint64_t *d_w = s.d_weights + 4 * (size_t)(s.W + s.K);
    if (s.zk_kt) return zkx_compose_launch(ctx, s.XD, s.SH, s.H, (uint32_t)s.cfg->trace_offset, s.log_n, s.zk_kt, s.d_lde, N, s.d_cl, N, d_w, s.d_cw, N);
    if (s.A) SMI_TRY(xargs_compose_enqueue(ctx, s.XD, s.SH, s.H, (uint32_t)s.cfg->trace_offset, s.d_lde, N, s.d_cl, N, d_w, s.d_cw, N));
    return SMI_OK;
}

// the coefficients of every coordinate of H on the coset
int deep_h_coefficients(DeepProver &s) { return dev_ntt(s.ctx, s.d_cw, s.d_hc, s.log_N, s.N, 4, s.N, s.N, 1, s.cfg->lde_offset, 1); }

// the segments: D slices of n of those coefficients, each extended back to the N points
int deep_segments(DeepProver &s) {
    SMI_TRY(deep_h_coefficients(s));
    for (uint32_t j = 0; j < s.D; j++)
        SMI_TRY(dev_ntt(s.ctx, s.d_hc + (size_t)j * s.n, s.d_seg + 4 * (size_t)j * s.N, s.log_N, s.n, 4, s.N, s.N, 0, s.cfg->lde_offset, 1));
    return SMI_OK;
}

// the round trip of the segments' root -> z
int deep_draw_z(DeepProver &s, uint8_t *roots_out) {
    smi_ctx *ctx = s.ctx;
    const uint32_t k = s.G - 1;
    HIP_TRY(ctx, deep_root_read(s, k));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t zr[4];
    if (s.A) deep_args_transcript_z(s.tr, s.roots + 32 * k, s.NW, zr);
    else deep_transcript_z(s.tr, s.roots + 32 * k, s.W, s.K, zr);
    s.z = fqh_of(zr, s.p);
    if (fqh_in_base(s.z)) return smi_fail(ctx, SMI_ERR_BAD_ARG, DEEP_Z_IN_BASE_FIELD);
    if (roots_out) memcpy(roots_out, s.roots, 32 * (size_t)s.G);
    return SMI_OK;
}

// the record: u, v = f(z), f(z w) of the trace (under a window: u_s = f(z w^s), s < S); a, b = c(z), c(z w) of the auxiliary
// columns; s_j = the segments at z.
// Coordinate e of the D segments is D columns of n coefficients at d_src + e src_pitch, src_stride apart.
int deep_values_at_z(DeepProver &s, const uint32_t *d_src, size_t src_pitch, size_t src_stride, uint64_t *ood_out) {
    smi_ctx *ctx = s.ctx;
    const uint32_t W = s.W, A = s.A, CW = s.CW, D = s.D, p = s.p, g = s.g, S = s.S;
    const size_t n = s.n, PS = 4 * (size_t)S;   // words a column in the result
    FqH pts[SMI_AIR_MAX_WINDOW];
    pts[0] = s.z;
    for (uint32_t k = 1; k < S; k++) pts[k] = fqh_scale(pts[k - 1], s.w_n, p);
    std::vector<uint32_t> tab2, tab1, res(PS * (W + CW) + 16 * (size_t)D);
    deep_eval_build(ctx->fs.F, g, S, pts, &tab2);
    deep_eval_build(ctx->fs.F, g, 1, pts, &tab1);
    HIP_TRY(ctx, hipMemcpyAsync(s.d_tab2, tab2.data(), tab2.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(s.d_tab1, tab1.data(), tab1.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(deep_eval_enqueue(ctx, s.d_coef, W + CW, n, n, S, s.d_tab2, s.d_part, s.d_res));
    uint32_t *d_sres = s.d_res + PS * (W + CW);
    for (uint32_t e = 0; e < 4; e++) SMI_TRY(deep_eval_enqueue(ctx, d_src + e * src_pitch, D, n, src_stride, 1, s.d_tab1, s.d_part, d_sres + 4 * (size_t)e * D));
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), s.d_res, res.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    s.ood.assign(s.n_ood, 0);
    uint64_t *ood = s.ood.data();
    const FqH X{{0, 1 % p, 0, 0}};
    auto assemble = [&](const uint32_t *at, size_t pitch, uint64_t *dst) {   // sum_e X^e v_e, v_e four words at at + e pitch
        FqH sum = fqh(0), xe = fqh(1 % p);
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t *v = at + e * pitch;
            sum = fqh_add(sum, fqh_mul(xe, FqH{{v[0], v[1], v[2], v[3]}}, p, g), p);
            xe = fqh_mul(xe, X, p, g);
        }
        for (uint32_t e = 0; e < 4; e++) dst[e] = sum.c[e];
    };
    for (uint32_t k = 0; k < S; k++)   // s-major: u_{k,c} at 4 (k W + c)
        for (uint32_t c = 0; c < W; c++)
            for (uint32_t e = 0; e < 4; e++) ood[4 * ((size_t)k * W + c) + e] = res[PS * c + 4 * k + e];
    for (uint32_t a = 0; a < A; a++) {   // S = 2.  Coordinate column 4 a + e at z: res[8 (W + 4 a + e) ..], at z w: four words on
        assemble(&res[8 * (size_t)(W + 4 * a)], 8, &ood[4 * (2 * (size_t)W + a)]);
        assemble(&res[8 * (size_t)(W + 4 * a) + 4], 8, &ood[4 * (2 * (size_t)W + A + a)]);
    }
    for (uint32_t j = 0; j < D; j++) assemble(&res[PS * (W + CW) + 4 * (size_t)j], 4 * (size_t)D, &ood[4 * ((size_t)S * W + 2 * (size_t)A + j)]);
    if (ood_out) memcpy(ood_out, ood, 8 * s.n_ood);
    return SMI_OK;
}

// the record -> the gammas and FRI's seed; the DEEP codeword Q into d_cw
int deep_codeword(DeepProver &s) {
    smi_ctx *ctx = s.ctx;
    const uint32_t W = s.W, A = s.A, D = s.D, h = (uint32_t)s.cfg->lde_offset;
    const size_t N = s.N;
    std::vector<uint64_t> gammas;
    if (A) deep_args_transcript_gammas(s.tr, s.ood.data(), s.NW, s.n_ood, &gammas);
    else deep_transcript_gammas(s.tr, s.ood.data(), W, s.K, D, &gammas, s.S);
    s.seed = s.tr.seed();
    if (A) deep_compose_args_build(ctx->fs.F, s.g, W, A, D, s.w_n, s.z, s.ood.data(), gammas.data(), &s.ctab);
    else deep_compose_build(ctx->fs.F, s.g, W, D, s.w_n, s.z, s.ood.data(), gammas.data(), &s.ctab, s.S);
    HIP_TRY(ctx, hipMemcpyAsync(s.d_ctab, s.ctab.data(), s.ctab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if (A) return deep_compose_args_enqueue(ctx, W, A, D, s.log_N, h, s.d_ctab, s.d_lde, N, s.d_cl, N, s.d_seg, N, s.d_cw, N);
    return deep_compose_enqueue(ctx, W, D, s.log_N, h, s.d_ctab, s.d_lde, N, s.d_seg, N, s.d_cw, N, s.S);
}

// the head of the proof: tag 2 | the record's length | its values
void deep_record_header(DeepProver &s) {
    std::vector<uint8_t> &bytes = s.bytes;
    bytes.assign(9 + 8 * s.n_ood, 0);
    bytes[0] = 2;
    for (int i = 0; i < 8; i++) bytes[1 + i] = (uint8_t)((uint64_t)s.n_ood >> (8 * i));
    for (size_t v = 0; v < s.n_ood; v++)
        for (int i = 0; i < 8; i++) bytes[9 + 8 * v + i] = (uint8_t)(s.ood[v] >> (8 * i));
}

// FRI over the codeword where it stands (stride N: no compaction copy); the proof so far: header | FRI's stream
int deep_fri(DeepProver &s, uint32_t grind_bits, uint64_t *top_indices) {
    smi_ctx *ctx = s.ctx;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, s.cfg, 1ull << s.cfg->log_blowup);
    if (s.cosets) SMI_TRY(fri_run_ext_fold4(ctx, &fc, &s.seed, s.d_cw, s.N, s.N, false, &s.fri, grind_bits));
    else SMI_TRY(fri_run_ext(ctx, &fc, &s.seed, s.d_cw, s.N, s.N, false, &s.fri, (int)grind_bits));
    deep_record_header(s);
    s.bytes.insert(s.bytes.end(), s.fri.proof.begin(), s.fri.proof.end());
    if (top_indices) memcpy(top_indices, s.fri.top.data(), 8 * (size_t)s.cfg->num_colinearity_tests);
    return SMI_OK;
}

// every group at FRI's top-level indices, appended to the proof: row leaves by one launch a group (R = 2 rows a test), coset
// leaves by one launch for all groups (one leaf and one path per test and group)
int deep_open(DeepProver &s) {
    smi_ctx *ctx = s.ctx;
    const uint32_t t = (uint32_t)s.cfg->num_colinearity_tests, R = 2, log_N = s.log_N;
    if (!t) return SMI_OK;
    size_t at[3] = {0, 0, 0}, total = 0;   // group k's section in the openings
    for (uint32_t k = 0; k < s.G; k++) {
        at[k] = total;
        total += s.cosets ? (size_t)mg_coset_open_bytes(s.V[k], t, log_N) : (size_t)mg_row_open_bytes(s.V[k], t, log_N, R);
    }
    uint64_t *d_top = (uint64_t *)arena_alloc(ctx, 8 * (size_t)t);
    uint8_t *d_open = (uint8_t *)arena_alloc(ctx, total);
    if (!d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, (std::string(s.name) + (s.cosets ? ": coset openings" : ": row openings")).c_str());
    HIP_TRY(ctx, hipMemcpyAsync(d_top, s.fri.top.data(), 8 * (size_t)t, hipMemcpyHostToDevice, ctx->stream));
    if (s.cosets) {
        MgCosetTable tab;
        memset(&tab, 0, sizeof tab);
        for (uint32_t k = 0; k < s.G; k++) tab.g[k] = MgCosetGroup{s.cols[k], s.N, s.tree[k], at[k], s.V[k], 0};
        coset_open_kernel<<<dim3(t, s.G), 64, 0, ctx->stream>>>(tab, log_N, d_top, t, d_open);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        for (uint32_t k = 0; k < s.G; k++)
            SMI_TRY(launch_air_row_open(ctx, s.cols[k], s.N, s.V[k], s.tree[k], log_N, d_top, t, R, 1ull << s.cfg->log_blowup, d_open + at[k]));
    }
    const size_t end = s.bytes.size();
    s.bytes.resize(end + total);
    HIP_TRY(ctx, hipMemcpyAsync(s.bytes.data() + end, d_open, total, hipMemcpyDeviceToHost, ctx->stream));
    return SMI_OK;
}

// the last mark, the prover's final wait, the stage times and the proof
int deep_finish(DeepProver &s, uint8_t **proof, size_t *proof_len, double *stage_ms) {
    s.timer.mark();
    HIP_TRY(s.ctx, hipStreamSynchronize(s.ctx->stream));
    s.timer.write(stage_ms);
    return smi_proof_out(s.ctx, s.bytes, proof, proof_len);
}

// {row leaves, coset leaves} x {plain AIR (xargs == nullptr), argument list}
int deep_prove(smi_ctx *ctx, const char *name, bool cosets, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, const uint32_t *d_trace_cols,
               uint8_t *roots_out, uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits,
               uint32_t *closes) {
    if (closes) *closes = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(deep_field_check(ctx));
    uint32_t D = 0;
    {
        std::string why;
        const int rc = xargs ? deep_xargs_plan(ctx->fs.F.p, cfg, air, xargs, nullptr, &D, &why)
                             : deep_plan(ctx->fs.F.p, cfg, air, nullptr, &D, &why, SMI_AIR_MAX_WINDOW);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    DeepProver s(ctx, xargs ? 8 : 7, stage_ms != nullptr);
    s.cfg = cfg, s.air = air, s.xargs = xargs, s.name = name, s.cosets = cosets, s.d_trace = d_trace_cols;
    SMI_TRY(deep_shapes(s, D, DEEP_FOLD4_NO_LAYER));
    SMI_TRY(deep_setup(s));
    s.timer.mark();
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, s.W, s.log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, s.d_lde));
    s.timer.mark();
    SMI_TRY(deep_commit(s, 0));
    s.timer.mark();
    SMI_TRY(deep_root1(s));
    if (xargs) SMI_TRY(deep_list_columns(s, closes));   // marks the auxiliary stage
    else deep_transcript_weights(s.tr, s.roots, s.W, s.K, &s.weights);
    SMI_TRY(deep_compose_h(s));
    s.timer.mark();
    SMI_TRY(deep_segments(s));
    SMI_TRY(deep_commit(s, s.G - 1));
    s.timer.mark();
    SMI_TRY(deep_draw_z(s, roots_out));
    SMI_TRY(deep_values_at_z(s, s.d_hc, s.N, s.n, ood_out));
    SMI_TRY(deep_codeword(s));
    s.timer.mark();
    SMI_TRY(deep_fri(s, grind_bits, top_indices));
    s.timer.mark();
    SMI_TRY(deep_open(s));
    return deep_finish(s, proof, proof_len, stage_ms);
}

// ---- zero-knowledge DEEP proofs (include/stark_mi.h, "Zero-knowledge DEEP proofs")
// The coset-leaf plain prover with the four changes of the section, each a step of zk_prove: the last k_t rows of the trace
// overwritten in place and the derived AIR composed in the caller's place; the masked split (zk_segments_kernel) for the
// slices of n; the mask polynomial R extended with the segments and added to the DEEP codeword by zk_mask_add_kernel; one
// salt column in each tree.  Every random value comes from smi_dev_random_fill under the caller's seed and one of the
// ZK_STREAM_* identifiers.
struct ZkBuffers {
    uint32_t *d_rows, *d_rho, *d_sc;   // the randomiser rows; the split's masks; n coefficients a column: 4 D' of the segments, 4 of R
};

// the randomisers: column c takes elements c k_t .. (c + 1) k_t - 1 of their stream in its last k_t rows; the two salts
int zk_randomise(DeepProver &s, const uint8_t seed[32], uint32_t kt, const ZkBuffers &zb, uint32_t *d_trace_cols) {
    smi_ctx *ctx = s.ctx;
    const size_t n = s.n, N = s.N;
    SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_ROWS, zb.d_rows, (size_t)s.W * kt));
    HIP_TRY(ctx, hipMemcpy2DAsync(d_trace_cols + (n - kt), n * 4, zb.d_rows, (size_t)kt * 4, (size_t)kt * 4, s.W, hipMemcpyDeviceToDevice, ctx->stream));
    SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_SALT1, s.d_lde + (size_t)s.W * N, N));
    SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_SALT2, s.d_seg + (size_t)(s.V[s.G - 1] - 1) * N, N));
    return SMI_OK;
}

// the masked segments (D_h: the segments of H before masking) and R as coefficients, then one batched extension a polynomial
int zk_segments(DeepProver &s, const uint8_t seed[32], uint32_t D_h, uint32_t ks, const ZkBuffers &zb) {
    smi_ctx *ctx = s.ctx;
    const uint32_t Dp = s.D;
    const size_t n = s.n, N = s.N;
    SMI_TRY(deep_h_coefficients(s));
    if (Dp > 1) SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_RHO, zb.d_rho, (size_t)4 * (Dp - 1) * ks));
    SMI_TRY(smi_dev_zk_segments(ctx, s.d_hc, N, (size_t)D_h * n, s.log_n, ks, Dp, zb.d_rho, zb.d_sc, n));
    SMI_TRY(smi_dev_random_fill(ctx, seed, ZK_STREAM_MASK, zb.d_sc + (size_t)4 * Dp * n, 4 * n));
    for (uint32_t c = 0; c < s.V[s.G - 1] - 1; c += 4)
        SMI_TRY(dev_ntt(ctx, zb.d_sc + (size_t)c * n, s.d_seg + (size_t)c * N, s.log_N, n, 4, n, N, 0, s.cfg->lde_offset, 1));
    return SMI_OK;
}

// a plain AIR (xargs == nullptr: "Zero-knowledge DEEP proofs", nine stages) or an argument list ("... with an argument list",
// ten stages: the auxiliary columns' between commit and compose)
int zk_prove(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air0, const smi_air_xargs *xargs, uint32_t *d_trace_cols, const uint8_t seed[32],
             uint8_t *roots_out, uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits,
             uint32_t *closes) {
    if (closes) *closes = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(deep_field_check(ctx));
    uint32_t D_h = 0, Dp = 0, kt = 0, ks = 0;
    std::string why;
    int rc = xargs ? zkx_plan(ctx->fs.F.p, cfg, air0, xargs, nullptr, &Dp, &kt, &ks, &why, &D_h) : zk_plan(ctx->fs.F.p, cfg, air0, nullptr, &Dp, &kt, &ks, &why, &D_h);
    if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    DeepProver s(ctx, xargs ? 10 : 9, stage_ms != nullptr);
    s.cfg = cfg, s.air = air0, s.xargs = xargs, s.name = xargs ? "air_prove_deep_zk_xargs" : "air_prove_deep_zk", s.cosets = true, s.d_trace = d_trace_cols;
    SMI_TRY(deep_shapes(s, Dp, xargs ? ZKX_NO_LAYER : ZK_NO_LAYER));   // a list is checked against the caller's AIR
    const DeepGroups gr = xargs ? zkx_groups(s.W, s.A, Dp) : zk_groups(s.W, Dp);   // every tree with its salt column; the segments with R
    for (uint32_t k = 0; k < 3; k++) s.V[k] = gr.V[k];
    if (xargs) s.NW = s.W + s.K + 3 * s.A, s.zk_kt = kt, s.zk_seed = seed;
    ZkAir Z;
    rc = zk_derive_air(s.p, s.w_n, cfg, air0, &Z, &why, xargs != nullptr);
    if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    s.air = &Z.air;   // K stays the caller's: the weights are drawn for the caller's constraints
    SMI_TRY(deep_setup(s));
    const uint32_t segw = s.V[s.G - 1] - 1;   // 4 D' + 4: the segments' and R's columns
    ZkBuffers zb;
    zb.d_rows = (uint32_t *)arena_alloc(ctx, (size_t)s.W * kt * 4);
    zb.d_rho = (uint32_t *)arena_alloc(ctx, (size_t)4 * Dp * ks * 4);
    zb.d_sc = (uint32_t *)arena_alloc(ctx, (size_t)segw * s.n * 4);
    if (xargs) s.d_tail = (uint32_t *)arena_alloc(ctx, (size_t)s.CW * (kt - 1) * 4);
    if (!zb.d_rows || !zb.d_rho || !zb.d_sc || (xargs && !s.d_tail)) return smi_fail(ctx, SMI_ERR_OOM, (std::string(s.name) + ": device memory").c_str());
    s.timer.mark();
    SMI_TRY(zk_randomise(s, seed, kt, zb, d_trace_cols));
    s.timer.mark();
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, s.W, s.log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, s.d_lde));
    s.timer.mark();
    SMI_TRY(deep_commit(s, 0));
    s.timer.mark();
    SMI_TRY(deep_root1(s));
    if (xargs) SMI_TRY(deep_list_columns(s, closes));   // marks the auxiliary stage
    else deep_transcript_weights(s.tr, s.roots, s.W, s.K, &s.weights);
    SMI_TRY(deep_compose_h(s));
    s.timer.mark();
    SMI_TRY(zk_segments(s, seed, D_h, ks, zb));
    SMI_TRY(deep_commit(s, s.G - 1));
    s.timer.mark();
    SMI_TRY(deep_draw_z(s, roots_out));
    SMI_TRY(deep_values_at_z(s, zb.d_sc, s.n, 4 * s.n, ood_out));   // the masked segments: coordinate e of segment j is column 4 j + e
    SMI_TRY(deep_codeword(s));
    s.timer.mark();
    SMI_TRY(zk_mask_add_launch(ctx, s.d_cw, s.N, s.d_seg + (size_t)4 * Dp * s.N, s.N, s.N));   // Q' = Q + R
    s.timer.mark();
    SMI_TRY(deep_fri(s, grind_bits, top_indices));
    s.timer.mark();
    SMI_TRY(deep_open(s));
    return deep_finish(s, proof, proof_len, stage_ms);
}
}  // namespace

int smi_dev_air_prove_deep(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t *roots_out, uint64_t *ood_out,
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return deep_prove(ctx, "air_prove_deep", false, cfg, (const smi_air *)air, nullptr, d_trace_cols, roots_out, ood_out, proof, proof_len, top_indices, stage_ms,
                      grind_bits, nullptr);
}
int smi_dev_air_prove_deep_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint32_t *d_trace_cols, uint8_t *roots_out,
                                 uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits,
                                 uint32_t *closes) {
    if (!ctx || !cfg || !air || !xargs || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return deep_prove(ctx, "air_prove_deep_xargs", false, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, d_trace_cols, roots_out, ood_out, proof,
                      proof_len, top_indices, stage_ms, grind_bits, closes);
}
int smi_dev_air_prove_deep_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t *roots_out, uint64_t *ood_out,
                                 uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return deep_prove(ctx, "air_prove_deep_fold4", true, cfg, (const smi_air *)air, nullptr, d_trace_cols, roots_out, ood_out, proof, proof_len, top_indices,
                      stage_ms, grind_bits, nullptr);
}
int smi_dev_air_prove_deep_xargs_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint32_t *d_trace_cols,
                                       uint8_t *roots_out, uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms,
                                       uint32_t grind_bits, uint32_t *closes) {
    if (!ctx || !cfg || !air || !xargs || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return deep_prove(ctx, "air_prove_deep_fold4", true, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, d_trace_cols, roots_out, ood_out, proof,
                      proof_len, top_indices, stage_ms, grind_bits, closes);
}
int smi_dev_air_prove_deep_zk(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, uint32_t *d_trace_cols, const uint8_t seed[32], uint8_t *roots_out,
                              uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !d_trace_cols || !seed || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return zk_prove(ctx, cfg, (const smi_air *)air, nullptr, d_trace_cols, seed, roots_out, ood_out, proof, proof_len, top_indices, stage_ms, grind_bits,
                    nullptr);
}
int smi_dev_air_prove_deep_zk_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint32_t *d_trace_cols, const uint8_t seed[32],
                                    uint8_t *roots_out, uint64_t *ood_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms,
                                    uint32_t grind_bits, uint32_t *closes) {
    if (!ctx || !cfg || !air || !xargs || !d_trace_cols || !seed || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return zk_prove(ctx, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, d_trace_cols, seed, roots_out, ood_out, proof, proof_len, top_indices,
                    stage_ms, grind_bits, closes);
}

