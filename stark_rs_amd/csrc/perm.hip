// perm.hip -- the permutation argument over a committed extension column (include/stark_mi.h, "Permutation argument"):
// the column z by batched F_q division and a device-wide prefix product, the two auxiliary quotients added into the
// composition codeword, and the prover with its second commitment round.  The lane bodies are perm_core.h, shared with the
// CPU emulator (emu_perm.cpp); the verifier is in verify.hip.
//
// The column build is a multi-launch scan, with no wait of one workgroup on another:
//   perm_block_kernel      a lane takes PERM_ROWS consecutive rows, forms f_L and f_R, inverts its denominators with one F_q
//                          inversion and multiplies up its rho; the workgroup scans the lane products in LDS; every row
//                          gets its prefix WITHIN the workgroup (stored to z, Montgomery form) and the workgroup its product;
//   perm_scan_kernel       one workgroup loops over the workgroup products, PERM_BLOCK at a time, and leaves exclusive
//                          prefixes (plain) in their place, and the total;
//   perm_propagate_kernel  z[r] = prefix of r's workgroup * stored value: one F_q product per row.
// The third launch reloads the stored prefixes rather than recomputing the ratios: a row's ratio costs the two tuples,
// 3.25 F_q products and a quarter of an inversion, the reload 32 bytes of traffic and one product (DESIGN.md has the figures).
// One tile of perm_scan_kernel covers PERM_BLOCK * PERM_TILE = 2^18 rows; above that it loops.
//
// (perm_load4 / perm_store4, the 16-byte accesses of these kernels, are row4_dev.h's, shared with lookup.hip.)
//
// air_perm_compose_kernel streams: per lane four consecutive points, one 16-byte load per tuple column, two per
// coordinate of z (this row, and B further: a second coalesced read, no halo), a 16-byte read-modify-write per coordinate of
// the codeword.  x_i advances by a per-lane step over a grid-stride loop, so the two powers a lane computes are set-up.
#include <string>
#include <vector>

#include "air_core.h"
#include "hash_core.h"
#include "internal.h"
#include "mgpu_core.h"
#include "perm_core.h"
#include "row4_dev.h"

namespace {
// the workgroup scan of perm_core.h (perm_scan_step) between barriers; returns the lane's EXCLUSIVE prefix and the
// workgroup's product.  sc: 2 x 4 x PERM_BLOCK words of LDS.
__device__ __forceinline__ Fq perm_wg_scan(Fq v, uint32_t (*sc)[4][PERM_BLOCK], uint32_t tid, uint32_t g_m, const Fp &F, Fq *total) {
    __syncthreads();   // the buffers of the scan before are consumed
#pragma unroll
    for (int e = 0; e < 4; e++) sc[0][e][tid] = v.c[e];
    __syncthreads();
    int cur = 0;
    for (uint32_t off = 1; off < PERM_BLOCK; off <<= 1) {
        perm_scan_step(sc[cur], sc[cur ^ 1], tid, off, g_m, F);
        __syncthreads();
        cur ^= 1;
    }
    *total = perm_scan_at(sc[cur], PERM_BLOCK - 1);
    return tid ? perm_scan_at(sc[cur], tid - 1) : fq_one(F);
}
}  // namespace

template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void perm_block_kernel(PermDev PD, Fp F, const uint32_t *__restrict__ trace, uint64_t n, uint32_t *__restrict__ z,
                                                                 size_t z_stride, uint32_t *__restrict__ block_prod, unsigned long long *first) {
    __shared__ uint32_t sc[2][4][PERM_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint64_t row0 = ((uint64_t)blockIdx.x * PERM_BLOCK + tid) * PERM_ROWS;
    Fq zl[PERM_ROWS], prod;
    uint64_t zero_row;
    perm_lane_column(
        PD, F, row0, n,
        [&](uint32_t col, uint32_t v[4]) {
            if (row0 < n) perm_load4<VEC>(trace + (uint64_t)col * n, row0, n, v);
            else v[0] = v[1] = v[2] = v[3] = 0u;
        },
        zl, &prod, &zero_row);
    if (zero_row != ~0ull) atomicMin(first, (unsigned long long)zero_row);
    Fq total;
    const Fq excl = perm_wg_scan(prod, sc, tid, PD.g_m, F, &total);
    if (!tid) *(uint4 *)(block_prod + 4 * (uint64_t)blockIdx.x) = make_uint4(total.c[0], total.c[1], total.c[2], total.c[3]);
    if (row0 >= n) return;
    uint32_t o[4][PERM_ROWS];
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) {
        const Fq w = fq_mul(zl[q], excl, PD.g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) o[e][q] = w.c[e];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) perm_store4<VEC>(z + e * z_stride, row0, n, o[e]);
}

// bp: nb workgroup products (Montgomery, four words each) -> their exclusive prefixes (plain); total: the product of all
__global__ __launch_bounds__(PERM_BLOCK) void perm_scan_kernel(Fp F, uint32_t g_m, uint32_t nb, uint32_t *__restrict__ bp, uint32_t *__restrict__ total) {
    __shared__ uint32_t sc[2][4][PERM_BLOCK];
    const uint32_t tid = threadIdx.x;
    Fq carry = fq_one(F);
    for (uint32_t base = 0; base < nb; base += PERM_BLOCK) {   // wave-uniform trip count
        const bool in = base + tid < nb;
        Fq v = fq_one(F);
        if (in) {
            const uint4 t = *(const uint4 *)(bp + 4 * (uint64_t)(base + tid));
            v = Fq{{t.x, t.y, t.z, t.w}};
        }
        Fq tile;
        const Fq excl = perm_wg_scan(v, sc, tid, g_m, F, &tile);
        if (in) {
            const Fq w = fq_mul(carry, excl, g_m, F);
            *(uint4 *)(bp + 4 * (uint64_t)(base + tid)) = make_uint4(from_mont(w.c[0], F), from_mont(w.c[1], F), from_mont(w.c[2], F), from_mont(w.c[3], F));
        }
        carry = fq_mul(carry, tile, g_m, F);
    }
    if (!tid) *(uint4 *)total = make_uint4(from_mont(carry.c[0], F), from_mont(carry.c[1], F), from_mont(carry.c[2], F), from_mont(carry.c[3], F));
}

template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void perm_propagate_kernel(Fp F, uint32_t g_m, uint64_t n, uint32_t *__restrict__ z, size_t z_stride,
                                                                     const uint32_t *__restrict__ block_excl) {
    const uint64_t row0 = ((uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x) * PERM_ROWS;
    if (row0 >= n) return;
    const uint4 t = *(const uint4 *)(block_excl + 4 * (uint64_t)blockIdx.x);   // wave-uniform
    const uint32_t pre[4] = {t.x, t.y, t.z, t.w};
    const ExtMul M = ext_mul_prepare(pre, g_m, F);   // plain: (stored Montgomery value) * M is plain
    uint32_t v[4][PERM_ROWS];
#pragma unroll
    for (int e = 0; e < 4; e++) perm_load4<VEC>(z + e * z_stride, row0, n, v[e]);
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) {
        const uint32_t a[4] = {v[0][q], v[1][q], v[2][q], v[3][q]};
        uint32_t o[4];
        ext_mul_prepared(a, M, F, o);
#pragma unroll
        for (int e = 0; e < 4; e++) v[e][q] = o[e];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) perm_store4<VEC>(z + e * z_stride, row0, n, v[e]);
}

// out (four coordinate columns, the composition of the main AIR) += w_b * boundary quotient + w_t * transition quotient of z
template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void air_perm_compose_kernel(PermDev PD, Fp F, uint64_t N, uint32_t log_B, uint32_t h_m, uint32_t omega_m,
                                                                       uint32_t tau_m, const uint32_t *__restrict__ izt_m, const uint32_t *__restrict__ lde,
                                                                       size_t stride, const uint32_t *__restrict__ zl, size_t z_stride,
                                                                       const uint64_t *__restrict__ w, uint32_t *__restrict__ out, size_t out_stride) {
    uint32_t wm[4];
#pragma unroll
    for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[e], F);
    const ExtMul wb = ext_mul_prepare(wm, PD.g_m, F);
#pragma unroll
    for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[4 + e], F);
    const ExtMul wt = ext_mul_prepare(wm, PD.g_m, F);
    const uint64_t groups = N / PERM_ROWS, gid = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x, gstep = (uint64_t)gridDim.x * PERM_BLOCK;
    const uint32_t B = 1u << log_B;
    uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * PERM_ROWS, F), F);
    const uint32_t xstep_m = mont_pow(omega_m, gstep * PERM_ROWS, F);
    for (uint64_t g = gid; g < groups; g += gstep) {
        const uint64_t i0 = g * PERM_ROWS, i1 = (i0 + B) & (N - 1);   // B and N are multiples of 4: no access straddles the wrap
        uint32_t zc[4][PERM_ROWS], zx[4][PERM_ROWS], acc[4][PERM_ROWS];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            perm_load4<VEC>(zl + e * z_stride, i0, N, zc[e]);
            perm_load4<VEC>(zl + e * z_stride, i1, N, zx[e]);
            perm_load4<VEC>(out + e * out_stride, i0, N, acc[e]);
        }
        perm_compose_points(
            PD, F, wb, wt, tau_m, izt_m, B, i0, x_m, omega_m, [&](uint32_t col, uint32_t v[4]) { perm_load4<VEC>(lde + (uint64_t)col * stride, i0, N, v); }, zc, zx,
            acc);
#pragma unroll
        for (int e = 0; e < 4; e++) perm_store4<VEC>(out + e * out_stride, i0, N, acc[e]);
        x_m = mont_mul(x_m, xstep_m, F);
    }
}

namespace {
// bytes of device scratch the column build wants: the workgroup products | the total (16) | the first zero row (8, padded)
size_t perm_column_tmp_bytes(uint64_t n) { return ((n + PERM_TILE - 1) / PERM_TILE) * 16 + 32; }

struct PermFlags {   // as the column build leaves them on the device: total (4 words, plain), first zero row
    uint32_t total[4];
    unsigned long long first;
    unsigned long long pad;
};

// the three launches; d_tmp: perm_column_tmp_bytes(n) bytes, 16-byte aligned.  The flags are at d_tmp + nb * 16.
int perm_column_enqueue(smi_ctx *ctx, const PermDev &PD, const uint32_t *d_trace, uint32_t log_n, uint32_t *d_z, size_t z_stride, uint8_t *d_tmp) {
    const uint64_t n = 1ull << log_n, nb = (n + PERM_TILE - 1) / PERM_TILE;
    uint32_t *d_bp = (uint32_t *)d_tmp;
    PermFlags *d_fl = (PermFlags *)(d_tmp + nb * 16);
    const Fp F = ctx->fs.F;
    const bool vec = n >= 4 && al16(d_trace) && al16(d_z) && !(z_stride & 3);
    HIP_TRY(ctx, hipMemsetAsync(&d_fl->first, 0xff, 8, ctx->stream));
    {
        ProfScope ps(ctx, "perm_block_kernel", (4.0 * 2 * PD.m + 16.0) * (double)n);
        if (vec) perm_block_kernel<true><<<(uint32_t)nb, PERM_BLOCK, 0, ctx->stream>>>(PD, F, d_trace, n, d_z, z_stride, d_bp, &d_fl->first);
        else perm_block_kernel<false><<<(uint32_t)nb, PERM_BLOCK, 0, ctx->stream>>>(PD, F, d_trace, n, d_z, z_stride, d_bp, &d_fl->first);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, "perm_scan_kernel", 32.0 * (double)nb);
        perm_scan_kernel<<<1, PERM_BLOCK, 0, ctx->stream>>>(F, PD.g_m, (uint32_t)nb, d_bp, d_fl->total);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, "perm_propagate_kernel", 32.0 * (double)n);
        if (vec) perm_propagate_kernel<true><<<(uint32_t)nb, PERM_BLOCK, 0, ctx->stream>>>(F, PD.g_m, n, d_z, z_stride, d_bp);
        else perm_propagate_kernel<false><<<(uint32_t)nb, PERM_BLOCK, 0, ctx->stream>>>(F, PD.g_m, n, d_z, z_stride, d_bp);
        HIP_TRY(ctx, hipGetLastError());
    }
    return SMI_OK;
}
const PermFlags *perm_column_flags(const uint8_t *d_tmp, uint32_t log_n) { return (const PermFlags *)(d_tmp + (((1ull << log_n) + PERM_TILE - 1) / PERM_TILE) * 16); }

// the verdicts of a finished column build (fl: the flags copied to the host)
int perm_column_verdict(smi_ctx *ctx, const PermFlags &fl, int *closes) {
    if (fl.first != ~0ull) {
        const std::string why = "perm_column: f_R is zero in row " + std::to_string(fl.first) + ": no inverse";
        return smi_fail(ctx, SMI_ERR_NO_INVERSE, why.c_str());
    }
    if (closes) *closes = fl.total[0] == 1u && !(fl.total[1] | fl.total[2] | fl.total[3]);
    return SMI_OK;
}

// H bound to the device blob (air_compose_ext_launch leaves it so)
int perm_compose_enqueue(smi_ctx *ctx, const PermDev &PD, const AirHost &H, uint32_t tau, const uint32_t *d_lde, size_t stride, const uint32_t *d_zl,
                         size_t z_stride, const uint64_t *d_w8, uint32_t *d_out, size_t out_stride) {
    const AirDev &A = H.dev;
    const Fp F = ctx->fs.F;
    const bool vec = al16(d_lde) && al16(d_zl) && al16(d_out) && !(stride & 3) && !(z_stride & 3) && !(out_stride & 3);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK, cap = (uint64_t)ctx->num_cus * 8;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint32_t tau_m = air_to_m(tau, F.p);
    ProfScope ps(ctx, "air_perm_compose_kernel", (4.0 * 2 * PD.m + 32.0 + 32.0) * (double)A.N);
    if (vec)
        air_perm_compose_kernel<true><<<grid, PERM_BLOCK, 0, ctx->stream>>>(PD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, A.izt_m, d_lde, stride, d_zl, z_stride,
                                                                            d_w8, d_out, out_stride);
    else
        air_perm_compose_kernel<false><<<grid, PERM_BLOCK, 0, ctx->stream>>>(PD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, A.izt_m, d_lde, stride, d_zl, z_stride,
                                                                             d_w8, d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int perm_args(smi_ctx *ctx, const smi_air_perm *perm, uint32_t n_cols, uint32_t log_n) {
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "perm: modulus must be < 2^30");
    std::string why;
    if (!n_cols || n_cols > 64) return smi_fail(ctx, SMI_ERR_BAD_ARG, "perm: 1..64 columns");
    if (log_n < 1 || log_n > 27) return smi_fail(ctx, SMI_ERR_BAD_ARG, "perm: log_n must be in 1 .. 27");
    if (perm_validate(perm, n_cols, &why) != SMI_OK) return smi_fail(ctx, SMI_ERR_BAD_ARG, why.c_str());
    return SMI_OK;
}
}  // namespace

int smi_dev_perm_column(smi_ctx *ctx, const void *perm_, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, const uint64_t *challenges,
                        uint32_t *d_z, size_t z_stride, int *closes) {
    const smi_air_perm *perm = (const smi_air_perm *)perm_;
    if (!ctx || !perm || !d_trace_cols || !challenges || !d_z) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(perm_args(ctx, perm, n_cols, log_n));
    if (z_stride < (1ull << log_n)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "perm_column: z_stride < n");
    PermDev PD;
    perm_build(ctx->fs.F, ctx->fs.g, perm, challenges, &PD);
    void *tmp = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, perm_column_tmp_bytes(1ull << log_n), &tmp));
    SMI_TRY(perm_column_enqueue(ctx, PD, d_trace_cols, log_n, d_z, z_stride, (uint8_t *)tmp));
    PermFlags fl;
    HIP_TRY(ctx, hipMemcpyAsync(&fl, perm_column_flags((const uint8_t *)tmp, log_n), sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return perm_column_verdict(ctx, fl, closes);
}

int smi_dev_air_compose_perm(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *perm_, const uint32_t *d_lde, size_t stride,
                             const uint32_t *d_z_lde, size_t z_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                             size_t out_stride) {
    const smi_air_perm *perm = (const smi_air_perm *)perm_;
    if (!ctx || !cfg || !air || !perm || !d_lde || !d_z_lde || !challenges || !d_weights || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    AirHost H;
    SMI_TRY(air_host_tables(ctx, cfg, (const smi_air *)air, &H, nullptr));
    SMI_TRY(perm_args(ctx, perm, cfg->n_cols, cfg->log_n));
    if (stride < H.dev.N || out_stride < H.dev.N || z_stride < H.dev.N)
        return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_perm: stride < N, z_stride < N or out_stride < N");
    const size_t b_tab = up16(H.per.table_words * 4), b_vals = up16(H.per.vals.size() * 4);
    void *base = nullptr;   // tables | grouped values | blob
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_vals + H.blob.size() * 4, &base));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, (uint32_t *)((uint8_t *)base + b_tab), (uint32_t *)base));
    SMI_TRY(air_compose_ext_launch(ctx, H, (uint32_t *)((uint8_t *)base + b_tab + b_vals), d_lde, stride, d_weights, d_out, out_stride));
    PermDev PD;
    perm_build(ctx->fs.F, ctx->fs.g, perm, challenges, &PD);
    const uint32_t W = cfg->n_cols, K = ((const smi_air *)air)->n_constraints;
    return perm_compose_enqueue(ctx, PD, H, (uint32_t)cfg->trace_offset, d_lde, stride, d_z_lde, z_stride, d_weights + 4 * (size_t)(W + K), d_out, out_stride);
}

int smi_dev_air_prove_perm(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const void *perm_, const uint32_t *d_trace_cols, uint8_t *roots_out,
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, int *closes) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_perm *perm = (const smi_air_perm *)perm_;
    if (!ctx || !cfg || !air || !perm || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    AirHost H;
    uint64_t E = 0;
    SMI_TRY(air_host_tables(ctx, cfg, air, &H, &E));   // E of the AIR: the auxiliary constraints of degree 2 leave D as it is
    SMI_TRY(perm_args(ctx, perm, cfg->n_cols, cfg->log_n));
    {
        std::string why;
        const int rc = perm_plan(ctx->fs.F.p, cfg, air, perm, nullptr, &E, &why);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    const size_t n = (size_t)1 << cfg->log_n, N = n << cfg->log_blowup;
    PermDev PD;
    TwoTreeVariant v;
    v.name = "air_prove_perm";
    v.A = 1;
    v.tmp_bytes = perm_column_tmp_bytes(n);
    v.flags_bytes = sizeof(PermFlags);
    v.columns = [&](const uint64_t *ch, const uint32_t *, uint32_t *d_z, uint8_t *d_tmp) {
        perm_build(ctx->fs.F, ctx->fs.g, perm, ch, &PD);
        return perm_column_enqueue(ctx, PD, d_trace_cols, cfg->log_n, d_z, n, d_tmp);
    };
    v.settle = [&](const void *fl) { return perm_column_verdict(ctx, *(const PermFlags *)fl, closes); };
    v.compose = [&](const AirHost &Hd, const uint32_t *d_lde, const uint32_t *d_zl, const uint64_t *d_w, uint32_t *d_cw) {
        return perm_compose_enqueue(ctx, PD, Hd, (uint32_t)cfg->trace_offset, d_lde, N, d_zl, N, d_w, d_cw, N);
    };
    return two_tree_prove(ctx, cfg, H, E, d_trace_cols, v, roots_out, proof, proof_len, top_indices, stage_ms, grind_bits);
}

// The prover of every proof with two row trees (internal.h TwoTreeVariant): smi_dev_air_prove_perm, _lookup, _args and _xargs
// behind their checks and plans.  Two waits of the host before FRI, one per root; the order of the arena's allocations fixes
// the alignment of every buffer, and the six stage marks are those of the header's stage_ms lists.
int two_tree_prove(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, uint64_t E, const uint32_t *d_trace_cols, const TwoTreeVariant &v, uint8_t *roots_out,
                   uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    const uint32_t W = cfg->n_cols, K = H.dev.K, log_n = cfg->log_n, log_N = cfg->log_n + cfg->log_blowup;
    const size_t n = (size_t)1 << log_n, N = (size_t)1 << log_N;
    const uint32_t NW = W + K + 2 * v.A, CW = 4 * v.A;   // weights; coordinate columns of the second tree
    const std::string name = v.name;
    SMI_TRY(arena_reset(ctx));
    StageTimer tm(ctx, 6, stage_ms != nullptr);
    HIP_TRY(ctx, tm.create());

    const size_t tree_bytes = 2 * N * 32;
    uint32_t *d_lde = (uint32_t *)arena_alloc(ctx, (size_t)W * N * 4);
    uint32_t *d_c = (uint32_t *)arena_alloc(ctx, (size_t)CW * n * 4);
    uint32_t *d_cl = (uint32_t *)arena_alloc(ctx, (size_t)CW * N * 4);
    uint32_t *d_cw = (uint32_t *)arena_alloc(ctx, 4 * N * 4);
    uint64_t *d_weights = (uint64_t *)arena_alloc(ctx, 8 * 4 * (size_t)NW);
    uint32_t *d_blob = (uint32_t *)arena_alloc(ctx, H.blob.size() * 4);
    uint8_t *tree1 = (uint8_t *)arena_alloc(ctx, tree_bytes), *tree2 = (uint8_t *)arena_alloc(ctx, tree_bytes);
    uint8_t *d_tmp = (uint8_t *)arena_alloc(ctx, v.tmp_bytes);
    uint32_t *d_ptab = nullptr, *d_pvals = nullptr;
    if (H.dev.Q) {
        d_ptab = (uint32_t *)arena_alloc(ctx, H.per.table_words * 4);
        d_pvals = (uint32_t *)arena_alloc(ctx, H.per.vals.size() * 4);
    }
    if (!d_lde || !d_c || !d_cl || !d_cw || !d_weights || !d_blob || !tree1 || !tree2 || !d_tmp || (H.dev.Q && (!d_ptab || !d_pvals)))
        return smi_fail(ctx, SMI_ERR_OOM, (name + ": device memory").c_str());
    tm.mark();
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, W, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_lde));
    tm.mark();
    SMI_TRY(launch_merkle_rows(ctx, d_lde, W, N, N, tree1));
    tm.mark();
    // first round trip: root_1 -> alpha, gamma
    uint8_t roots[64];
    HIP_TRY(ctx, hipMemcpyAsync(roots, tree1 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, d_pvals, d_ptab));   // queued before the host waits for the root; d_pvals: the raw values a list's column build may read
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    Transcript tr;
    std::vector<uint64_t> ch, weights;   // 8 challenges; 4 NW weights
    transcript_perm_challenges(tr, roots, &ch);
    SMI_TRY(v.columns(ch.data(), d_pvals, d_c, d_tmp));
    SMI_TRY(smi_dev_lde(ctx, d_c, CW, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_cl));
    SMI_TRY(launch_merkle_rows(ctx, d_cl, CW, N, N, tree2));
    tm.mark();
    // second round trip: root_2 (and the columns' verdicts) -> the weights and FRI's seed
    alignas(8) uint8_t flags[sizeof(ArgsFlags)];
    HIP_TRY(ctx, hipMemcpyAsync(roots + 32, tree2 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(flags, d_tmp + v.tmp_bytes - v.flags_bytes, v.flags_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    SMI_TRY(v.settle(flags));
    transcript_args_weights(tr, roots + 32, W, K, v.A, &weights);   // with one column transcript_perm_weights' bytes
    const FsSeed seed = tr.seed();
    if (roots_out) memcpy(roots_out, roots, 64);
    HIP_TRY(ctx, hipMemcpyAsync(d_weights, weights.data(), 8 * weights.size(), hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(air_compose_ext_launch(ctx, H, d_blob, d_lde, N, d_weights, d_cw, N));
    SMI_TRY(v.compose(H, d_lde, d_cl, d_weights + 4 * (size_t)(W + K), d_cw));
    tm.mark();
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, E);
    FriExtResult xres;
    SMI_TRY(fri_run_ext(ctx, &fc, &seed, d_cw, N, N, false, &xres, (int)grind_bits));
    std::vector<uint8_t> &bytes = xres.proof;
    if (top_indices) memcpy(top_indices, xres.top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    tm.mark();
    if (cfg->num_colinearity_tests) {
        const uint32_t t = (uint32_t)cfg->num_colinearity_tests, R = 4;
        const size_t ob1 = (size_t)mg_row_open_bytes(W, t, log_N, R), ob2 = (size_t)mg_row_open_bytes(CW, t, log_N, R);
        uint64_t *d_top = (uint64_t *)arena_alloc(ctx, 8 * (size_t)t);
        uint8_t *d_open = (uint8_t *)arena_alloc(ctx, ob1 + ob2);
        if (!d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, (name + ": row openings").c_str());
        HIP_TRY(ctx, hipMemcpyAsync(d_top, xres.top.data(), 8 * (size_t)t, hipMemcpyHostToDevice, ctx->stream));
        SMI_TRY(launch_air_row_open(ctx, d_lde, N, W, tree1, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open));
        SMI_TRY(launch_air_row_open(ctx, d_cl, N, CW, tree2, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open + ob1));
        const size_t at = bytes.size();
        bytes.resize(at + ob1 + ob2);
        HIP_TRY(ctx, hipMemcpyAsync(bytes.data() + at, d_open, ob1 + ob2, hipMemcpyDeviceToHost, ctx->stream));
    }
    tm.mark();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    tm.write(stage_ms);
    return smi_proof_out(ctx, bytes, proof, proof_len);
}
