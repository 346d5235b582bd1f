// zk.hip -- the device side of zero-knowledge DEEP proofs (include/stark_mi.h, "Zero-knowledge DEEP proofs"): random residues
// from the project's hash in counter mode, and the masked split of the composition's coefficients.  The lane bodies and the
// host plan are zk_core.h, shared with the CPU emulator (emu_zk.cpp).
//
// random_fill_kernel  a lane hashes two block counters at once in the paired state the grinding search uses (9 mixes for
//                     both, no memory traffic but the stores, no LDS, no atomics) and stores its eight residues with two
//                     16-byte stores; the last lane of an odd count and an unaligned base store word by word.
// zk_segments_kernel  streams: a lane makes four consecutive coefficients of one output column from two 16-byte loads of H
//                     (its window starts at j L + m0, which is odd-aligned in general) and one 16-byte store; the k_s
//                     masked coefficients at either end of a column read rho with scalar-sized loads.  4 bytes read and 4
//                     written per coefficient, plus the window's overlap.
#include <string>

#include "internal.h"
#include "row4_dev.h"
#include "zk_core.h"

// deep.hip's deep_load4 restated: four consecutive words from `at` (a multiple of 4), 0 at and above len
template <bool VEC>
__device__ __forceinline__ void zk_load4(const uint32_t *__restrict__ src, uint64_t at, uint64_t len, uint32_t v[4]) {
    if (VEC && at + 4 <= len) {
        const uint4 t = *(const uint4 *)(src + at);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
    }
}

template <bool VEC>
__global__ __launch_bounds__(ZK_BLOCK) void random_fill_kernel(Fp F, ZkRandSeed S, uint32_t *__restrict__ out, uint64_t count) {
    const uint64_t lane = (uint64_t)blockIdx.x * ZK_BLOCK + threadIdx.x, at = lane * ZK_RAND_PER_LANE;
    if (at >= count) return;
    uint32_t v[ZK_RAND_PER_LANE];
    zk_rand_lane(S.mid, lane, F, v);
    if (VEC && at + ZK_RAND_PER_LANE <= count) {
        *(uint4 *)(out + at) = make_uint4(v[0], v[1], v[2], v[3]);
        *(uint4 *)(out + at + 4) = make_uint4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int q = 0; q < ZK_RAND_PER_LANE; q++)
            if (at + q < count) out[at + q] = v[q];
    }
}

// grid (groups of four coefficients, column 4 j + e)
template <bool VEC>
__global__ __launch_bounds__(ZK_BLOCK) void zk_segments_kernel(Fp F, ZkSegShape S, const uint32_t *__restrict__ hc, size_t h_stride,
                                                               const uint32_t *__restrict__ rho, uint32_t *__restrict__ out, size_t out_stride) {
    const uint64_t g = (uint64_t)blockIdx.x * ZK_BLOCK + threadIdx.x, m0 = 4 * g;
    if (m0 >= S.n) return;
    zk_seg_group(
        S, blockIdx.y, m0, hc, h_stride, rho, out, out_stride, F.p, [](const uint32_t *src, uint64_t at, uint64_t len, uint32_t v[4]) { zk_load4<VEC>(src, at, len, v); },
        [](uint32_t *dst, uint64_t at, uint64_t len, const uint32_t v[4]) { perm_store4<VEC>(dst, at, len, v); });
}

// Q' = Q + R on four coordinate columns, four points a lane
template <bool VEC>
__global__ __launch_bounds__(ZK_BLOCK) void zk_mask_add_kernel(uint32_t p, uint32_t *__restrict__ q, size_t q_stride, const uint32_t *__restrict__ r, size_t r_stride,
                                                               uint64_t N) {
    const uint64_t i0 = 4 * ((uint64_t)blockIdx.x * ZK_BLOCK + threadIdx.x);
    if (i0 >= N) return;
    const uint32_t e = blockIdx.y;
    uint32_t a[4], b[4];
    perm_load4<VEC>(q + e * q_stride, i0, N, a);
    perm_load4<VEC>(r + e * r_stride, i0, N, b);
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = fp_add(a[k], b[k], p);
    perm_store4<VEC>(q + e * q_stride, i0, N, a);
}
int zk_mask_add_launch(smi_ctx *ctx, uint32_t *d_q, size_t q_stride, const uint32_t *d_r, size_t r_stride, size_t N) {
    const bool vec = al16(d_q) && al16(d_r) && !(q_stride & 3) && !(r_stride & 3) && !(N & 3);
    const dim3 grid((uint32_t)((N / 4 + ZK_BLOCK - 1) / ZK_BLOCK), 4);   // N is a power of two >= 4
    ProfScope ps(ctx, "zk_mask_add_kernel", 48.0 * (double)N);
    if (vec) zk_mask_add_kernel<true><<<grid, ZK_BLOCK, 0, ctx->stream>>>(ctx->fs.F.p, d_q, q_stride, d_r, r_stride, N);
    else zk_mask_add_kernel<false><<<grid, ZK_BLOCK, 0, ctx->stream>>>(ctx->fs.F.p, d_q, q_stride, d_r, r_stride, N);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int smi_dev_random_fill(smi_ctx *ctx, const uint8_t seed[32], uint64_t stream_id, uint32_t *d_out, size_t count) {
    if (!ctx || !seed || (!d_out && count)) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if ((uint64_t)count > (1ull << 34)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "random_fill: at most 2^34 residues a call");
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "random_fill: modulus must be < 2^30 (the bias bound 2^-34)");
    if (!count) return SMI_OK;
    const ZkRandSeed S = zk_rand_seed(seed, stream_id);
    const uint64_t lanes = ((uint64_t)count + ZK_RAND_PER_LANE - 1) / ZK_RAND_PER_LANE;
    const uint32_t grid = (uint32_t)((lanes + ZK_BLOCK - 1) / ZK_BLOCK);   // <= 2^23
    ProfScope ps(ctx, "random_fill_kernel", 4.0 * (double)count, 9.0 * (double)lanes * 2.0);
    if (al16(d_out)) random_fill_kernel<true><<<grid, ZK_BLOCK, 0, ctx->stream>>>(ctx->fs.F, S, d_out, count);
    else random_fill_kernel<false><<<grid, ZK_BLOCK, 0, ctx->stream>>>(ctx->fs.F, S, d_out, count);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int smi_dev_zk_segments(smi_ctx *ctx, const uint32_t *d_h, size_t h_stride, size_t h_len, uint32_t log_n, uint32_t k_s, uint32_t n_segments,
                        const uint32_t *d_rho, uint32_t *d_out, size_t out_stride) {
    if (!ctx || !d_h || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (log_n < 2 || log_n > 27) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_segments: log_n must be in 2 .. 27");
    const uint64_t n = 1ull << log_n;
    if (!k_s || k_s >= n / 2) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_segments: k_s must be in 1 .. n / 2 - 1");
    if (!n_segments || 4 * n_segments + 5 > ZK_MAX_RECORD) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_segments: 1 .. 14 segments (4 D' + 5 <= 64)");
    if (n_segments > 1 && !d_rho) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_segments: more than one segment needs rho");
    const uint64_t L = n - k_s;
    if (h_stride < h_len || out_stride < n) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_segments: h_stride < h_len or out_stride < n");
    if ((uint64_t)h_len > (uint64_t)n_segments * L)
        return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_segments: h_len > D' (n - k_s): the segments do not hold every coefficient of H");
    const ZkSegShape S{n, L, (uint64_t)h_len, k_s, n_segments};
    const bool vec = al16(d_h) && al16(d_out) && !(h_stride & 3) && !(out_stride & 3);
    const dim3 grid((uint32_t)((n / 4 + ZK_BLOCK - 1) / ZK_BLOCK), 4 * n_segments);
    ProfScope ps(ctx, "zk_segments_kernel", 4.0 * ((double)h_len * 4 + 4.0 * n_segments * (double)n));
    if (vec) zk_segments_kernel<true><<<grid, ZK_BLOCK, 0, ctx->stream>>>(ctx->fs.F, S, d_h, h_stride, d_rho, d_out, out_stride);
    else zk_segments_kernel<false><<<grid, ZK_BLOCK, 0, ctx->stream>>>(ctx->fs.F, S, d_h, h_stride, d_rho, d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
