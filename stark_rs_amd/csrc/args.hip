// args.hip -- several permutation and lookup arguments in one proof (include/stark_mi.h, "Argument list"): the entry points of
// the plain list, and the scan and propagation launches every list's column build ends with.
//
// A plain list is an operand list without selectors or periodic members, and that is how it runs: each entry point makes its
// own checks with its own sentences (args_args, args_plan), converts the list on the host (xargs_core.h XArgsOfPlain) and
// hands it to what the operand list's entry points run behind their checks (xargs.hip: xargs_block_kernel,
// air_xargs_compose_kernel, the two-tree prover).  The AIR's periodic columns are not looked at on the way.
//   args_scan_kernel       A workgroups, one per argument, each looping over its argument's workgroup aggregates PERM_BLOCK
//                          at a time; leaves plain exclusive prefixes in their place, and the argument's total.
//   args_propagate_kernel  grid (workgroups of rows, A): one F_q product per row for a permutation, four additions for a
//                          lookup.
#include <string>
#include <vector>

#include "air_core.h"
#include "args_dev.h"
#include "hash_core.h"
#include "internal.h"
#include "mgpu_core.h"
#include "row4_dev.h"
#include "xargs_core.h"

// workgroup a: the nb aggregates of argument a -> their exclusive prefixes (plain); total + 4 a: the argument's total (plain)
__global__ __launch_bounds__(PERM_BLOCK) void args_scan_kernel(ArgsScanDev AD, Fp F, uint32_t nb, uint32_t *__restrict__ block_agg, uint32_t *__restrict__ total) {
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
__global__ __launch_bounds__(PERM_BLOCK) void args_propagate_kernel(ArgsScanDev AD, Fp F, uint64_t n, uint32_t *__restrict__ c, size_t c_stride,
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

static_assert(SMI_ARGS_MAX == 8, "ArgsFlags (internal.h) holds SMI_ARGS_MAX totals");
// the scan launch and the propagation launch of a column build whose block launch has filled d_c and d_agg
int args_scan_propagate_enqueue(smi_ctx *ctx, const ArgsScanDev &AD, uint64_t n, bool vec, uint32_t *d_c, size_t c_stride, uint32_t *d_agg, ArgsFlags *d_fl) {
    const uint64_t nb = (n + PERM_TILE - 1) / PERM_TILE;
    const uint32_t A = AD.A;
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
int args_args(smi_ctx *ctx, const smi_air_args *args, uint32_t n_cols, uint32_t log_n) {
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "args: modulus must be < 2^30");
    std::string why;
    if (!n_cols || n_cols > 64) return smi_fail(ctx, SMI_ERR_BAD_ARG, "args: 1..64 columns");
    if (log_n < 1 || log_n > 27) return smi_fail(ctx, SMI_ERR_BAD_ARG, "args: log_n must be in 1 .. 27");
    if (args_validate(args, n_cols, &why) != SMI_OK) return smi_fail(ctx, SMI_ERR_BAD_ARG, why.c_str());
    return SMI_OK;
}
const ListNames ARGS_NAMES = {"args_columns", "f_R", "air_prove_args"};
}  // namespace

int smi_dev_args_columns(smi_ctx *ctx, const void *args_, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, const uint64_t *challenges,
                         uint32_t *d_c, size_t c_stride, uint32_t *closes) {
    const smi_air_args *args = (const smi_air_args *)args_;
    if (!ctx || !args || !d_trace_cols || !challenges || !d_c) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(args_args(ctx, args, n_cols, log_n));
    if (c_stride < (1ull << log_n)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "args_columns: c_stride < n");
    const XArgsOfPlain x(args);
    return xargs_columns_run(ctx, nullptr, &x.list, ARGS_NAMES, d_trace_cols, n_cols, log_n, challenges, d_c, c_stride, closes);
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
    const XArgsOfPlain x(args);
    return xargs_compose_run(ctx, cfg, H, nullptr, &x.list, d_lde, stride, d_c_lde, c_stride, challenges, d_weights, d_out, out_stride);
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
    const XArgsOfPlain x(args);
    return xargs_prove_run(ctx, cfg, H, E, nullptr, &x.list, ARGS_NAMES, d_trace_cols, roots_out, proof, proof_len, top_indices, stage_ms, grind_bits, closes);
}
