// zkargs.hip -- the device side of zero-knowledge DEEP proofs with an argument list (include/stark_mi.h, "Zero-knowledge DEEP
// proofs with an argument list"): the tail step of the auxiliary columns and the three auxiliary quotients.  The lane bodies
// and the host plan are zkargs_core.h, shared with the CPU emulator (emu_zkargs.cpp); the prover is a driver in deep.hip, the
// verifier is in verify.hip.
//
// zk_args_tail_kernel           one launch for all 4 A coordinate columns, grid (groups of four words, column): row n_a of every
//                               column goes to the verdict flags, rows n_a + 1 .. n - 1 take the column's k_t - 1 random words.
//                               n_a + 1 is odd, so a column's first group is stored word by word, the groups behind it with one
//                               16-byte store each, the last one word by word again when the column's end cuts it.
// air_zk_xargs_compose_kernel   air_xargs_compose_kernel's streaming loop over zkx_compose_points: the E_A factor on the wrapping
//                               transition quotient and the closing quotient cq_a, 12 weight coordinates an argument.  A sibling
//                               of that kernel, which stays as it is.  E_A(x_i) is the derived AIR's extended periodic table
//                               Q + 1, read like any periodic operand.
#include <string>
#include <vector>

#include "air_core.h"
#include "internal.h"
#include "row4_dev.h"
#include "zkargs_core.h"

template <bool VEC>
__global__ __launch_bounds__(ZK_BLOCK) void zk_args_tail_kernel(ZkTailShape S, const uint32_t *__restrict__ rnd, uint32_t *c, size_t c_stride,
                                                                uint32_t *__restrict__ total) {
    const uint32_t col = blockIdx.y;
    const uint64_t grp = (uint64_t)blockIdx.x * ZK_BLOCK + threadIdx.x;
    if (!grp) total[col] = zk_tail_closing(S, col, c, c_stride);
    if (grp >= zk_tail_groups(S)) return;
    zk_tail_group(
        S, col, grp, VEC, rnd, c, c_stride, [](uint32_t *dst, const uint32_t v[4]) { *(uint4 *)dst = make_uint4(v[0], v[1], v[2], v[3]); },
        [](uint32_t *dst, uint32_t v) { *dst = v; });
}

// out (four coordinate columns, the composition of the derived AIR) += the 3 A auxiliary quotients under w (12 A coordinates)
// SHT: XNoShared (air_zk_xargs_compose_kernel) or XSharedDev (air_zk_xargs_compose_shared_kernel, a list with a shared lookup)
template <bool VEC, class SHT>
__device__ __forceinline__ void air_zk_xargs_compose_body(const XArgsDev &XD, const SHT &SH, const Fp &F, uint64_t N, uint32_t log_B, uint32_t h_m,
                                                          uint32_t omega_m, uint32_t tau_m, uint32_t tna_m, uint32_t ea_op, const uint32_t *__restrict__ izt_m,
                                                          const uint32_t *__restrict__ plog, const uint32_t *__restrict__ pofs, const uint32_t *__restrict__ ptab,
                                                          const uint32_t *__restrict__ lde, size_t stride, const uint32_t *__restrict__ cl, size_t c_stride,
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
        zkx_compose_points(
            XD, SH, F, w, tau_m, tna_m, ea_op, izt_m, B, i0, x_m, omega_m,
            [&](uint32_t op, uint32_t v[4]) {   // op is wave-uniform
                if (xop_periodic(op)) {
                    uint64_t L, at;
                    const uint32_t *table = xargs_table_at(plog, pofs, ptab, op & 0xffu, i0, &L, &at);
                    perm_load4<VEC>(table, at, L, v);
                } else {
                    perm_load4<VEC>(lde + (uint64_t)op * stride, i0, N, v);
                }
            },
            [&](uint32_t col, bool next, uint32_t v[4]) { perm_load4<VEC>(cl + (uint64_t)col * c_stride, next ? i1 : i0, N, v); }, acc);
#pragma unroll
        for (int e = 0; e < 4; e++) perm_store4<VEC>(out + e * out_stride, i0, N, acc[e]);
        x_m = mont_mul(x_m, xstep_m, F);
    }
}
template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void air_zk_xargs_compose_kernel(XArgsDev XD, Fp F, uint64_t N, uint32_t log_B, uint32_t h_m, uint32_t omega_m,
                                                                           uint32_t tau_m, uint32_t tna_m, uint32_t ea_op, const uint32_t *__restrict__ izt_m,
                                                                           const uint32_t *__restrict__ plog, const uint32_t *__restrict__ pofs,
                                                                           const uint32_t *__restrict__ ptab, const uint32_t *__restrict__ lde, size_t stride,
                                                                           const uint32_t *__restrict__ cl, size_t c_stride, const uint64_t *__restrict__ w,
                                                                           uint32_t *__restrict__ out, size_t out_stride) {
    air_zk_xargs_compose_body<VEC>(XD, XNoShared{}, F, N, log_B, h_m, omega_m, tau_m, tna_m, ea_op, izt_m, plog, pofs, ptab, lde, stride, cl, c_stride, w, out,
                                   out_stride);
}
template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void air_zk_xargs_compose_shared_kernel(XArgsDev XD, XSharedDev SH, Fp F, uint64_t N, uint32_t log_B, uint32_t h_m,
                                                                                  uint32_t omega_m, uint32_t tau_m, uint32_t tna_m, uint32_t ea_op,
                                                                                  const uint32_t *__restrict__ izt_m, const uint32_t *__restrict__ plog,
                                                                                  const uint32_t *__restrict__ pofs, const uint32_t *__restrict__ ptab,
                                                                                  const uint32_t *__restrict__ lde, size_t stride, const uint32_t *__restrict__ cl,
                                                                                  size_t c_stride, const uint64_t *__restrict__ w, uint32_t *__restrict__ out,
                                                                                  size_t out_stride) {
    air_zk_xargs_compose_body<VEC>(XD, SH, F, N, log_B, h_m, omega_m, tau_m, tna_m, ea_op, izt_m, plog, pofs, ptab, lde, stride, cl, c_stride, w, out, out_stride);
}

// d_total: 4 A words, word 4 a + e = coordinate e of c_a[n_a]; d_rnd: 4 A (k_t - 1) words
int zk_args_tail_launch(smi_ctx *ctx, uint32_t *d_c, size_t c_stride, uint32_t log_n, uint32_t kt, uint32_t A, const uint32_t *d_rnd, uint32_t *d_total) {
    const uint64_t n = 1ull << log_n;
    const ZkTailShape S{n, n - kt, kt, A};
    const dim3 grid((uint32_t)((zk_tail_groups(S) + ZK_BLOCK - 1) / ZK_BLOCK), 4 * A);
    ProfScope ps(ctx, "zk_args_tail_kernel", 8.0 * 4 * A * (double)(kt - 1));
    if (al16(d_c)) zk_args_tail_kernel<true><<<grid, ZK_BLOCK, 0, ctx->stream>>>(S, d_rnd, d_c, c_stride, d_total);
    else zk_args_tail_kernel<false><<<grid, ZK_BLOCK, 0, ctx->stream>>>(S, d_rnd, d_c, c_stride, d_total);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

// H: the DERIVED AIR's tables, bound to the device blob and its periodic tables (its last table is E_A's); d_w: the 12 A
// coordinates behind the main weights
int zkx_compose_launch(smi_ctx *ctx, const XArgsDev &XD, const XSharedDev *SH, const AirHost &H, uint32_t tau, uint32_t log_n, uint32_t kt, const uint32_t *d_lde, size_t stride, const uint32_t *d_cl,
                       size_t c_stride, const uint64_t *d_w, uint32_t *d_out, size_t out_stride) {
    const AirDev &A = H.dev;
    const Fp F = ctx->fs.F;
    if (A.log_B < 2) return smi_fail(ctx, SMI_ERR_EXPANSION_TOO_SMALL, "air_compose_zk_xargs: log_blowup < 2");
    if (A.Q < 2) return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_zk_xargs: the AIR is not a derived one");
    for (uint32_t j = 0; j < A.Q; j++)
        if (H.per.ofs[j] & ((1u << H.per.log_len[j]) - 1u))
            return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_zk_xargs: a periodic table does not start at a multiple of its length");
    const bool vec = al16(d_lde) && al16(d_cl) && al16(d_out) && !(stride & 3) && !(c_stride & 3) && !(out_stride & 3) && al16(A.ptab);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK, cap = (uint64_t)ctx->num_cus * 8;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint64_t n = 1ull << log_n;
    const uint32_t tau_m = air_to_m(tau, F.p), tna_m = air_to_m(host_mulmod(tau % F.p, host_powmod(h_root(ctx, log_n), n - kt, F.p), F.p), F.p);
    const uint32_t ea_op = XOP_PER | (A.Q - 1);
    double cols = 1 + (SH ? xshared_cols_read(XD, *SH) : 0);   // operands read per point, over the arguments, and E_A
    for (uint32_t a = 0; a < XD.A; a++)
        cols += 2 * XD.m[a] + (XD.kind[a] == SMI_ARG_LOOKUP ? 1 : 0) + (XD.asel[a] != SMI_ARG_NO_SELECTOR) + (XD.bsel[a] != SMI_ARG_NO_SELECTOR);
    ProfScope ps(ctx, SH ? "air_zk_xargs_compose_shared_kernel" : "air_zk_xargs_compose_kernel", (4.0 * cols + 32.0 * XD.A + 32.0) * (double)A.N);
    if (SH && vec)
        air_zk_xargs_compose_shared_kernel<true><<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, *SH, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, tna_m, ea_op, A.izt_m, A.plog,
                                                                                       A.pofs, A.ptab, d_lde, stride, d_cl, c_stride, d_w, d_out, out_stride);
    else if (SH)
        air_zk_xargs_compose_shared_kernel<false><<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, *SH, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, tna_m, ea_op, A.izt_m,
                                                                                        A.plog, A.pofs, A.ptab, d_lde, stride, d_cl, c_stride, d_w, d_out, out_stride);
    else if (vec)
        air_zk_xargs_compose_kernel<true><<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, tna_m, ea_op, A.izt_m, A.plog, A.pofs,
                                                                                A.ptab, d_lde, stride, d_cl, c_stride, d_w, d_out, out_stride);
    else
        air_zk_xargs_compose_kernel<false><<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, tna_m, ea_op, A.izt_m, A.plog,
                                                                                 A.pofs, A.ptab, d_lde, stride, d_cl, c_stride, d_w, d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int smi_dev_zk_args_tail(smi_ctx *ctx, uint32_t *d_c, size_t c_stride, uint32_t log_n, uint32_t k_t, uint32_t n_args, const uint32_t *d_rnd,
                         uint64_t *closing) {
    if (!ctx || !d_c || !d_rnd) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (log_n < 2 || log_n > 27) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_args_tail: log_n must be in 2 .. 27");
    const uint64_t n = 1ull << log_n;
    if (k_t < 2 || k_t >= n / 2 || (k_t & 7)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_args_tail: k_t must be a multiple of 8 in 8 .. n / 2 - 1");
    if (!n_args || n_args > SMI_ARGS_MAX) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_args_tail: 1 .. 8 auxiliary columns");
    if (c_stride < n) return smi_fail(ctx, SMI_ERR_BAD_ARG, "zk_args_tail: c_stride < n");
    void *tmp = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, 16 * SMI_ARGS_MAX, &tmp));
    SMI_TRY(zk_args_tail_launch(ctx, d_c, c_stride, log_n, k_t, n_args, d_rnd, (uint32_t *)tmp));
    if (!closing) return SMI_OK;
    uint32_t got[4 * SMI_ARGS_MAX];
    HIP_TRY(ctx, hipMemcpyAsync(got, tmp, 16 * (size_t)n_args, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < 4 * n_args; i++) closing[i] = got[i];
    return SMI_OK;
}

int smi_dev_air_compose_zk_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const void *xargs_, const uint32_t *d_lde, size_t stride,
                                 const uint32_t *d_c_lde, size_t c_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                                 size_t out_stride) {
    const smi_air *air0 = (const smi_air *)air_;
    const smi_air_xargs *xargs = (const smi_air_xargs *)xargs_;
    if (!ctx || !cfg || !air0 || !xargs || !d_lde || !d_c_lde || !challenges || !d_weights || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(ext_field_check(ctx));
    std::string why;
    uint32_t kt = 0;
    int rc = zkx_plan(ctx->fs.F.p, cfg, air0, xargs, nullptr, nullptr, &kt, nullptr, &why);
    if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    SMI_TRY(xargs_args(ctx, air0, xargs, cfg->n_cols, cfg->log_n));
    ZkAir Z;
    rc = zk_derive_air(ctx->fs.F.p, h_root(ctx, cfg->log_n), cfg, air0, &Z, &why, true);
    if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    AirHost H;
    SMI_TRY(air_host_tables(ctx, cfg, &Z.air, &H, nullptr));
    if (stride < H.dev.N || out_stride < H.dev.N || c_stride < H.dev.N)
        return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_zk_xargs: stride < N, c_stride < N or out_stride < N");
    const size_t b_tab = up16(H.per.table_words * 4), b_vals = up16(H.per.vals.size() * 4);
    void *base = nullptr;   // tables | grouped values | blob
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_vals + H.blob.size() * 4, &base));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, (uint32_t *)((uint8_t *)base + b_tab), (uint32_t *)base));
    SMI_TRY(air_compose_ext_launch(ctx, H, (uint32_t *)((uint8_t *)base + b_tab + b_vals), d_lde, stride, d_weights, d_out, out_stride));
    XArgsDev XD;
    xargs_build(ctx->fs.F, ctx->fs.g, xargs, cfg->n_cols, &Z.air, H.per, challenges, &XD);
    XSharedDev SHs;
    const XSharedDev *SH = xshared_build(xargs, cfg->n_cols, &SHs) ? &SHs : nullptr;
    const uint32_t W = cfg->n_cols, K = Z.air.n_constraints;
    SMI_TRY(zkx_compose_launch(ctx, XD, SH, H, (uint32_t)cfg->trace_offset, cfg->log_n, kt, d_lde, stride, d_c_lde, c_stride, d_weights + 4 * (size_t)(W + K), d_out, out_stride));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // Z and H are read by queued copies
    return SMI_OK;
}
