// args.hip -- several permutation and lookup arguments in one proof (include/stark_mi.h, "Argument list"): the A auxiliary
// columns by one trio of launches, the 2 A auxiliary quotients by one streaming launch, and the prover with its second
// commitment round over rows of 4 A values.  The lane bodies are args_core.h over perm_core.h and lookup_core.h, shared with
// the CPU emulator (emu_args.cpp); the verifier is in verify.hip.
//
// The column build is the multi-launch scan of perm.hip and lookup.hip with the argument as a grid dimension, so A arguments
// cost three launches and the latency of one scan workgroup:
//   args_block_kernel      grid (workgroups of rows, A).  A lane takes PERM_ROWS consecutive rows of argument blockIdx.y,
//                          forms its two tuples through the shared tables, inverts with one F_q inversion (perm_lane_ratios
//                          or lookup_lane_deltas) and the workgroup scans the lane aggregates in LDS: a product of Montgomery
//                          elements for a permutation, a sum of plain elements for a lookup.  The kind is uniform over the
//                          workgroup, so every barrier is met by all of its lanes.
//   args_scan_kernel       A workgroups, one per argument, each looping over its argument's workgroup aggregates PERM_BLOCK
//                          at a time; leaves plain exclusive prefixes in their place, and the argument's total.
//   args_propagate_kernel  grid (workgroups of rows, A): one F_q product per row for a permutation, four additions for a
//                          lookup.
// No look-back, no grid barrier, no spin; every loop is bounded by its data's size.
//
// air_args_compose_kernel streams as air_perm_compose_kernel does: per lane four consecutive points and ONE 16-byte
// read-modify-write per coordinate of the codeword whatever A is; the F_q accumulator stays in registers while the lane
// loops over the arguments, and 1 / (x - tau), the x_i walk and the 1 / (x^n - tau^n) entries are computed once per trip.
#include <string>
#include <vector>

#include "air_core.h"
#include "args_core.h"
#include "hash_core.h"
#include "internal.h"
#include "mgpu_core.h"
#include "row4_dev.h"

namespace {
// the workgroup scan of args_core.h (args_scan_step) between barriers; returns the lane's EXCLUSIVE prefix and the
// workgroup's aggregate.  sc: 2 x 4 x PERM_BLOCK words of LDS.  perm is uniform over the workgroup.
__device__ __forceinline__ Fq args_wg_scan(bool perm, Fq v, uint32_t (*sc)[4][PERM_BLOCK], uint32_t tid, uint32_t g_m, const Fp &F, Fq *total) {
    __syncthreads();   // the buffers of the scan before are consumed
#pragma unroll
    for (int e = 0; e < 4; e++) sc[0][e][tid] = v.c[e];
    __syncthreads();
    int cur = 0;
    for (uint32_t off = 1; off < PERM_BLOCK; off <<= 1) {
        args_scan_step(perm, sc[cur], sc[cur ^ 1], tid, off, g_m, F);
        __syncthreads();
        cur ^= 1;
    }
    *total = perm_scan_at(sc[cur], PERM_BLOCK - 1);
    return tid ? perm_scan_at(sc[cur], tid - 1) : args_identity(perm, F);
}
}  // namespace

// c: 4 A coordinate columns c_stride apart; block_agg: A runs of nb aggregates (four words each); first: the smallest key
template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void args_block_kernel(ArgsDev AD, Fp F, const uint32_t *__restrict__ trace, uint64_t n, uint32_t *__restrict__ c,
                                                                 size_t c_stride, uint32_t *__restrict__ block_agg, unsigned long long *first) {
    __shared__ uint32_t sc[2][4][PERM_BLOCK];
    const uint32_t tid = threadIdx.x, a = blockIdx.y;
    const bool perm = AD.kind[a] == SMI_ARG_PERM;
    const uint64_t row0 = ((uint64_t)blockIdx.x * PERM_BLOCK + tid) * PERM_ROWS;
    Fq pl[PERM_ROWS], agg;
    uint64_t key;
    args_lane_column(
        AD, a, F, row0, n,
        [&](uint32_t col, uint32_t v[4]) {
            if (row0 < n) perm_load4<VEC>(trace + (uint64_t)col * n, row0, n, v);
            else v[0] = v[1] = v[2] = v[3] = 0u;
        },
        pl, &agg, &key);
    if (key != ~0ull) atomicMin(first, (unsigned long long)key);
    Fq total;
    const Fq excl = args_wg_scan(perm, agg, sc, tid, AD.g_m, F, &total);
    if (!tid) *(uint4 *)(block_agg + 4 * ((uint64_t)a * gridDim.x + blockIdx.x)) = make_uint4(total.c[0], total.c[1], total.c[2], total.c[3]);
    if (row0 >= n) return;
    uint32_t o[4][PERM_ROWS];
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) {
        const Fq w = args_combine(perm, pl[q], excl, AD.g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) o[e][q] = w.c[e];
    }
    uint32_t *ca = c + 4 * (uint64_t)a * c_stride;
#pragma unroll
    for (int e = 0; e < 4; e++) perm_store4<VEC>(ca + e * c_stride, row0, n, o[e]);
}

// workgroup a: the nb aggregates of argument a -> their exclusive prefixes (plain); total + 4 a: the argument's total (plain)
__global__ __launch_bounds__(PERM_BLOCK) void args_scan_kernel(ArgsDev AD, Fp F, uint32_t nb, uint32_t *__restrict__ block_agg, uint32_t *__restrict__ total) {
    __shared__ uint32_t sc[2][4][PERM_BLOCK];
    const uint32_t tid = threadIdx.x, a = blockIdx.x;
    const bool perm = AD.kind[a] == SMI_ARG_PERM;
    uint32_t *bs = block_agg + 4 * (uint64_t)a * nb;
    Fq carry = args_identity(perm, F);
    for (uint32_t base = 0; base < nb; base += PERM_BLOCK) {   // wave-uniform trip count
        const bool in = base + tid < nb;
        Fq v = args_identity(perm, F);
        if (in) {
            const uint4 t = *(const uint4 *)(bs + 4 * (uint64_t)(base + tid));
            v = Fq{{t.x, t.y, t.z, t.w}};
        }
        Fq tile;
        const Fq excl = args_wg_scan(perm, v, sc, tid, AD.g_m, F, &tile);
        if (in) {
            const Fq w = args_scan_out(perm, args_combine(perm, carry, excl, AD.g_m, F), F);
            *(uint4 *)(bs + 4 * (uint64_t)(base + tid)) = make_uint4(w.c[0], w.c[1], w.c[2], w.c[3]);
        }
        carry = args_combine(perm, carry, tile, AD.g_m, F);
    }
    if (!tid) {
        const Fq w = args_scan_out(perm, carry, F);
        *(uint4 *)(total + 4 * a) = make_uint4(w.c[0], w.c[1], w.c[2], w.c[3]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void args_propagate_kernel(ArgsDev AD, Fp F, uint64_t n, uint32_t *__restrict__ c, size_t c_stride,
                                                                     const uint32_t *__restrict__ block_excl) {
    const uint32_t a = blockIdx.y;
    const uint64_t row0 = ((uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x) * PERM_ROWS;
    if (row0 >= n) return;
    const uint4 t = *(const uint4 *)(block_excl + 4 * ((uint64_t)a * gridDim.x + blockIdx.x));   // wave-uniform
    const uint32_t pre[4] = {t.x, t.y, t.z, t.w};
    uint32_t *ca = c + 4 * (uint64_t)a * c_stride;
    uint32_t v[4][PERM_ROWS];
#pragma unroll
    for (int e = 0; e < 4; e++) perm_load4<VEC>(ca + e * c_stride, row0, n, v[e]);
    args_propagate_rows(AD.kind[a] == SMI_ARG_PERM, pre, v, AD.g_m, F);
#pragma unroll
    for (int e = 0; e < 4; e++) perm_store4<VEC>(ca + e * c_stride, row0, n, v[e]);
}

// out (four coordinate columns, the composition of the main AIR) += the 2 A auxiliary quotients under w (8 A coordinates)
template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void air_args_compose_kernel(ArgsDev AD, Fp F, uint64_t N, uint32_t log_B, uint32_t h_m, uint32_t omega_m,
                                                                       uint32_t tau_m, const uint32_t *__restrict__ izt_m, const uint32_t *__restrict__ lde,
                                                                       size_t stride, const uint32_t *__restrict__ cl, size_t c_stride,
                                                                       const uint64_t *__restrict__ w, uint32_t *__restrict__ out, size_t out_stride) {
    const uint64_t groups = N / PERM_ROWS, gid = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x, gstep = (uint64_t)gridDim.x * PERM_BLOCK;
    const uint32_t B = 1u << log_B;
    uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * PERM_ROWS, F), F);
    const uint32_t xstep_m = mont_pow(omega_m, gstep * PERM_ROWS, F);
    for (uint64_t g = gid; g < groups; g += gstep) {
        const uint64_t i0 = g * PERM_ROWS, i1 = (i0 + B) & (N - 1);   // B and N are multiples of 4: no access straddles the wrap
        uint32_t acc[4][PERM_ROWS];
#pragma unroll
        for (int e = 0; e < 4; e++) perm_load4<VEC>(out + e * out_stride, i0, N, acc[e]);
        args_compose_points(
            AD, F, w, tau_m, izt_m, B, i0, x_m, omega_m, [&](uint32_t col, uint32_t v[4]) { perm_load4<VEC>(lde + (uint64_t)col * stride, i0, N, v); },
            [&](uint32_t col, bool next, uint32_t v[4]) { perm_load4<VEC>(cl + (uint64_t)col * c_stride, next ? i1 : i0, N, v); }, acc);
#pragma unroll
        for (int e = 0; e < 4; e++) perm_store4<VEC>(out + e * out_stride, i0, N, acc[e]);
        x_m = mont_mul(x_m, xstep_m, F);
    }
}

static_assert(SMI_ARGS_MAX == 8, "ArgsFlags (internal.h) holds SMI_ARGS_MAX totals");
// the scan launch and the propagation launch of a column build whose block launch has filled d_c and d_agg
int args_scan_propagate_enqueue(smi_ctx *ctx, const ArgsDev &AD, uint32_t A, uint64_t n, bool vec, uint32_t *d_c, size_t c_stride, uint32_t *d_agg,
                                ArgsFlags *d_fl) {
    const uint64_t nb = (n + PERM_TILE - 1) / PERM_TILE;
    const Fp F = ctx->fs.F;
    const dim3 grid((uint32_t)nb, A);
    {
        ProfScope ps(ctx, "args_scan_kernel", 32.0 * A * (double)nb);
        args_scan_kernel<<<A, PERM_BLOCK, 0, ctx->stream>>>(AD, F, (uint32_t)nb, d_agg, &d_fl->total[0][0]);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, "args_propagate_kernel", 32.0 * A * (double)n);
        if (vec) args_propagate_kernel<true><<<grid, PERM_BLOCK, 0, ctx->stream>>>(AD, F, n, d_c, c_stride, d_agg);
        else args_propagate_kernel<false><<<grid, PERM_BLOCK, 0, ctx->stream>>>(AD, F, n, d_c, c_stride, d_agg);
        HIP_TRY(ctx, hipGetLastError());
    }
    return SMI_OK;
}

namespace {
// bytes of device scratch the column build wants: A runs of workgroup aggregates | the flags
size_t args_columns_tmp_bytes(uint32_t A, uint64_t n) { return (size_t)A * ((n + PERM_TILE - 1) / PERM_TILE) * 16 + sizeof(ArgsFlags); }
const ArgsFlags *args_columns_flags(const uint8_t *d_tmp, uint32_t A, uint32_t log_n) {
    return (const ArgsFlags *)(d_tmp + (size_t)A * (((1ull << log_n) + PERM_TILE - 1) / PERM_TILE) * 16);
}

// the three launches; d_tmp: args_columns_tmp_bytes(A, n) bytes, 16-byte aligned
int args_columns_enqueue(smi_ctx *ctx, const ArgsDev &AD, const uint32_t *d_trace, uint32_t log_n, uint32_t *d_c, size_t c_stride, uint8_t *d_tmp) {
    const uint64_t n = 1ull << log_n, nb = (n + PERM_TILE - 1) / PERM_TILE;
    uint32_t *d_agg = (uint32_t *)d_tmp;
    ArgsFlags *d_fl = (ArgsFlags *)(d_tmp + (size_t)AD.A * nb * 16);
    const Fp F = ctx->fs.F;
    const bool vec = n >= 4 && al16(d_trace) && al16(d_c) && !(c_stride & 3);
    const dim3 grid((uint32_t)nb, AD.A);
    double cols = 0;   // trace columns read, over the arguments
    for (uint32_t a = 0; a < AD.A; a++) cols += 2 * AD.m[a] + (AD.kind[a] == SMI_ARG_LOOKUP ? 1 : 0);
    HIP_TRY(ctx, hipMemsetAsync(&d_fl->first, 0xff, 8, ctx->stream));
    {
        ProfScope ps(ctx, "args_block_kernel", (4.0 * cols + 16.0 * AD.A) * (double)n);
        if (vec) args_block_kernel<true><<<grid, PERM_BLOCK, 0, ctx->stream>>>(AD, F, d_trace, n, d_c, c_stride, d_agg, &d_fl->first);
        else args_block_kernel<false><<<grid, PERM_BLOCK, 0, ctx->stream>>>(AD, F, d_trace, n, d_c, c_stride, d_agg, &d_fl->first);
        HIP_TRY(ctx, hipGetLastError());
    }
    return args_scan_propagate_enqueue(ctx, AD, AD.A, n, vec, d_c, c_stride, d_agg, d_fl);
}

// the verdicts of a finished column build (fl: the flags copied to the host)
int args_columns_verdict(smi_ctx *ctx, const ArgsDev &AD, const ArgsFlags &fl, uint32_t *closes) {
    if (fl.first != ~0ull) {
        const uint32_t a = (uint32_t)(fl.first & 15) >> 1;
        const char *side = !(fl.first & 1) ? "f_L" : AD.kind[a] == SMI_ARG_PERM ? "f_R" : "f_T";
        const std::string why = "args_columns: argument " + std::to_string(a) + ": " + side + " is zero in row " + std::to_string(fl.first >> 4) + ": no inverse";
        return smi_fail(ctx, SMI_ERR_NO_INVERSE, why.c_str());
    }
    uint32_t mask = 0;
    for (uint32_t a = 0; a < AD.A; a++) {
        const uint32_t *t = fl.total[a];
        if (t[0] == (AD.kind[a] == SMI_ARG_PERM ? 1u : 0u) && !(t[1] | t[2] | t[3])) mask |= 1u << a;
    }
    if (closes) *closes = mask;
    return SMI_OK;
}

// H bound to the device blob (air_compose_ext_launch leaves it so); d_w: the 8 A coordinates behind the main weights
int args_compose_enqueue(smi_ctx *ctx, const ArgsDev &AD, const AirHost &H, uint32_t tau, const uint32_t *d_lde, size_t stride, const uint32_t *d_cl,
                         size_t c_stride, const uint64_t *d_w, uint32_t *d_out, size_t out_stride) {
    const AirDev &A = H.dev;
    const Fp F = ctx->fs.F;
    const bool vec = al16(d_lde) && al16(d_cl) && al16(d_out) && !(stride & 3) && !(c_stride & 3) && !(out_stride & 3);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK, cap = (uint64_t)ctx->num_cus * 8;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint32_t tau_m = air_to_m(tau, F.p);
    double cols = 0;
    for (uint32_t a = 0; a < AD.A; a++) cols += 2 * AD.m[a] + (AD.kind[a] == SMI_ARG_LOOKUP ? 1 : 0);
    ProfScope ps(ctx, "air_args_compose_kernel", (4.0 * cols + 32.0 * AD.A + 32.0) * (double)A.N);
    if (vec)
        air_args_compose_kernel<true><<<grid, PERM_BLOCK, 0, ctx->stream>>>(AD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, A.izt_m, d_lde, stride, d_cl, c_stride,
                                                                            d_w, d_out, out_stride);
    else
        air_args_compose_kernel<false><<<grid, PERM_BLOCK, 0, ctx->stream>>>(AD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, A.izt_m, d_lde, stride, d_cl, c_stride,
                                                                             d_w, d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int args_args(smi_ctx *ctx, const smi_air_args *args, uint32_t n_cols, uint32_t log_n) {
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "args: modulus must be < 2^30");
    std::string why;
    if (!n_cols || n_cols > 64) return smi_fail(ctx, SMI_ERR_BAD_ARG, "args: 1..64 columns");
    if (log_n < 1 || log_n > 27) return smi_fail(ctx, SMI_ERR_BAD_ARG, "args: log_n must be in 1 .. 27");
    if (args_validate(args, n_cols, &why) != SMI_OK) return smi_fail(ctx, SMI_ERR_BAD_ARG, why.c_str());
    return SMI_OK;
}
}  // namespace

int smi_dev_args_columns(smi_ctx *ctx, const void *args_, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, const uint64_t *challenges,
                         uint32_t *d_c, size_t c_stride, uint32_t *closes) {
    const smi_air_args *args = (const smi_air_args *)args_;
    if (!ctx || !args || !d_trace_cols || !challenges || !d_c) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(args_args(ctx, args, n_cols, log_n));
    if (c_stride < (1ull << log_n)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "args_columns: c_stride < n");
    ArgsDev AD;
    args_build(ctx->fs.F, ctx->fs.g, args, challenges, &AD);
    void *tmp = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, args_columns_tmp_bytes(AD.A, 1ull << log_n), &tmp));
    SMI_TRY(args_columns_enqueue(ctx, AD, d_trace_cols, log_n, d_c, c_stride, (uint8_t *)tmp));
    ArgsFlags fl;
    HIP_TRY(ctx, hipMemcpyAsync(&fl, args_columns_flags((const uint8_t *)tmp, AD.A, log_n), sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return args_columns_verdict(ctx, AD, fl, closes);
}

int smi_dev_air_compose_args(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *args_, const uint32_t *d_lde, size_t stride,
                             const uint32_t *d_c_lde, size_t c_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                             size_t out_stride) {
    const smi_air_args *args = (const smi_air_args *)args_;
    if (!ctx || !cfg || !air || !args || !d_lde || !d_c_lde || !challenges || !d_weights || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    AirHost H;
    SMI_TRY(air_host_tables(ctx, cfg, (const smi_air *)air, &H, nullptr));
    SMI_TRY(args_args(ctx, args, cfg->n_cols, cfg->log_n));
    if (stride < H.dev.N || out_stride < H.dev.N || c_stride < H.dev.N)
        return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_args: stride < N, c_stride < N or out_stride < N");
    const size_t b_tab = up16(H.per.table_words * 4), b_vals = up16(H.per.vals.size() * 4);
    void *base = nullptr;   // tables | grouped values | blob
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_vals + H.blob.size() * 4, &base));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, (uint32_t *)((uint8_t *)base + b_tab), (uint32_t *)base));
    SMI_TRY(air_compose_ext_launch(ctx, H, (uint32_t *)((uint8_t *)base + b_tab + b_vals), d_lde, stride, d_weights, d_out, out_stride));
    ArgsDev AD;
    args_build(ctx->fs.F, ctx->fs.g, args, challenges, &AD);
    const uint32_t W = cfg->n_cols, K = ((const smi_air *)air)->n_constraints;
    return args_compose_enqueue(ctx, AD, H, (uint32_t)cfg->trace_offset, d_lde, stride, d_c_lde, c_stride, d_weights + 4 * (size_t)(W + K), d_out, out_stride);
}

int smi_dev_air_prove_args(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const void *args_, const uint32_t *d_trace_cols, uint8_t *roots_out,
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, uint32_t *closes) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_args *args = (const smi_air_args *)args_;
    if (!ctx || !cfg || !air || !args || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    AirHost H;
    uint64_t E = 0;
    SMI_TRY(air_host_tables(ctx, cfg, air, &H, &E));   // E of the AIR alone; the plan below counts the auxiliary transitions in
    SMI_TRY(args_args(ctx, args, cfg->n_cols, cfg->log_n));
    {
        std::string why;
        const int rc = args_plan(ctx->fs.F.p, cfg, air, args, nullptr, &E, &why);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    const uint32_t W = cfg->n_cols, K = air->n_constraints, log_n = cfg->log_n, log_N = cfg->log_n + cfg->log_blowup, A = args->count;
    const size_t n = (size_t)1 << log_n, N = (size_t)1 << log_N;
    const uint32_t NW = W + K + 2 * A, CW = 4 * A;   // weights; coordinate columns of the second tree
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
    uint8_t *d_atmp = (uint8_t *)arena_alloc(ctx, args_columns_tmp_bytes(A, n));
    uint32_t *d_ptab = nullptr, *d_pvals = nullptr;
    if (H.dev.Q) {
        d_ptab = (uint32_t *)arena_alloc(ctx, H.per.table_words * 4);
        d_pvals = (uint32_t *)arena_alloc(ctx, H.per.vals.size() * 4);
    }
    if (!d_lde || !d_c || !d_cl || !d_cw || !d_weights || !d_blob || !tree1 || !tree2 || !d_atmp || (H.dev.Q && (!d_ptab || !d_pvals)))
        return smi_fail(ctx, SMI_ERR_OOM, "air_prove_args: device memory");
    tm.mark();
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, W, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_lde));
    tm.mark();
    SMI_TRY(launch_merkle_rows(ctx, d_lde, W, N, N, tree1));
    tm.mark();
    // first round trip: root_1 -> alpha, gamma
    uint8_t roots[64];
    HIP_TRY(ctx, hipMemcpyAsync(roots, tree1 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, d_pvals, d_ptab));   // queued before the host waits for the root
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    Transcript tr;
    std::vector<uint64_t> ch, weights;   // 8 challenges; 4 NW weights
    transcript_perm_challenges(tr, roots, &ch);
    ArgsDev AD;
    args_build(ctx->fs.F, ctx->fs.g, args, ch.data(), &AD);
    SMI_TRY(args_columns_enqueue(ctx, AD, d_trace_cols, log_n, d_c, n, d_atmp));
    SMI_TRY(smi_dev_lde(ctx, d_c, CW, log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_cl));
    SMI_TRY(launch_merkle_rows(ctx, d_cl, CW, N, N, tree2));
    tm.mark();
    // second round trip: root_2 (and the columns' verdicts) -> the weights and FRI's seed
    ArgsFlags fl;
    HIP_TRY(ctx, hipMemcpyAsync(roots + 32, tree2 + (2 * N - 2) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&fl, args_columns_flags(d_atmp, A, log_n), sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    SMI_TRY(args_columns_verdict(ctx, AD, fl, closes));
    transcript_args_weights(tr, roots + 32, W, K, A, &weights);
    const FsSeed seed = tr.seed();
    if (roots_out) memcpy(roots_out, roots, 64);
    HIP_TRY(ctx, hipMemcpyAsync(d_weights, weights.data(), 8 * weights.size(), hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(air_compose_ext_launch(ctx, H, d_blob, d_lde, N, d_weights, d_cw, N));
    SMI_TRY(args_compose_enqueue(ctx, AD, H, (uint32_t)cfg->trace_offset, d_lde, N, d_cl, N, d_weights + 4 * (size_t)(W + K), d_cw, N));
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
        if (!d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, "air_prove_args: row openings");
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
