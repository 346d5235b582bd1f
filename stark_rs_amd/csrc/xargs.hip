// xargs.hip -- the argument list with selectors and periodic members (include/stark_mi.h, "Argument list with selectors and
// periodic members"): the multiplicity helper over operands, the A auxiliary columns, the 2 A auxiliary quotients and the
// prover.  The lane bodies are xargs_core.h over args_core.h, shared with the CPU emulator (emu_xargs.cpp); the verifier is
// in verify.hip.  The plain list of args.hip ("Argument list") runs these kernels too: it is a list without selectors or
// periodic members, converted on the host (xargs_core.h XArgsOfPlain) behind its own checks.
//
// The column build is the multi-launch scan of perm.hip and lookup.hip with the argument as a grid dimension, so A arguments
// cost three launches and the latency of one scan workgroup:
//   xargs_block_kernel     grid (workgroups of rows, A).  A lane takes PERM_ROWS consecutive rows of argument blockIdx.y and
//                          forms its two tuples through the operand loader: a trace operand is one 16-byte load, a periodic
//                          operand four values v_j[(row0 + q) mod P_j] of the raw periodic values (one 16-byte load when
//                          P_j >= 4: row0 is a multiple of 4, so it cannot straddle the wrap; word by word when P_j is 1 or
//                          2).  The selectors are applied around perm_lane_ratios, a lookup goes through
//                          xlookup_lane_deltas: one F_q inversion per lane.  The workgroup scans the lane aggregates in LDS:
//                          a product of Montgomery elements for a permutation, a sum of plain elements for a lookup.  The
//                          kind is uniform over the workgroup, so every barrier is met by all of its lanes.
//   args_scan_kernel, args_propagate_kernel   (args.hip) they read kind[a] and nothing of the tuples.
// No look-back, no grid barrier, no spin; every loop is bounded by its data's size.
//
// air_xargs_compose_kernel streams as air_perm_compose_kernel does: per lane four consecutive points and ONE 16-byte
// read-modify-write per coordinate of the codeword whatever A is; the F_q accumulator stays in registers while the lane
// loops over the arguments, and 1 / (x - tau), the x_i walk and the 1 / (x^n - tau^n) entries are computed once per trip.
// A periodic operand is read at the lane's four points from the extended tables the main composition of the same call has
// built (AirDev::ptab), modulo L_j = P_j B.
// The helper is lookup.hip's two launches with rows that are not selected left out.
#include <string>
#include <vector>

#include "air_core.h"
#include "args_dev.h"
#include "hash_core.h"
#include "internal.h"
#include "mgpu_core.h"
#include "row4_dev.h"
#include "xargs_core.h"

namespace {
struct XDevAtomics {   // DevAtomics of lookup.hip
    __device__ __forceinline__ uint32_t cas(uint32_t *a, uint32_t expect, uint32_t v) const { return atomicCAS(a, expect, v); }
    __device__ __forceinline__ void min(uint32_t *a, uint32_t v) const { atomicMin(a, v); }
    // Lanes of a wave that arrive here together and count into the same word send ONE atomic with their sum.  Each trip
    // retires the first lane still here and every lane with its address: at most 64 trips, and no lane waits for a lane that
    // is not in the trip.
    __device__ __forceinline__ void add(uint32_t *a, uint32_t v) const {
        const uint64_t mine = (uint64_t)(uintptr_t)a;
        for (int trip = 0; trip < 64; trip++) {
            const uint32_t lead_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(mine >> 32)), lead_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)mine);
            const uint64_t lead = ((uint64_t)lead_hi << 32) | lead_lo;
            const uint64_t peers = __ballot(mine == lead);
            if (mine == lead) {
                if ((uint32_t)__lane_id() == (uint32_t)__ffsll((long long)peers) - 1) atomicAdd(a, v * (uint32_t)__popcll(peers));
                return;
            }
        }
    }
};
struct XHelperFlags {   // the first missing selected row, a probe that ran out
    unsigned long long first;
    uint32_t exhausted, pad;
};
}  // namespace

// rows <= n: the rows that take part (smi_dev_xargs_multiplicities_rows); the column stride stays n
// NEXT: the list has a next-row operand ("Argument list: next-row operands") -- a cell of such an operand is read at
// (row + 1) mod n by both launches, so both sides hash and compare the shifted values.  Every other list takes NEXT = false,
// whose cells look at no flag.
template <bool NEXT>
__global__ __launch_bounds__(PERM_BLOCK) void xargs_insert_kernel(XArgsDev XD, uint32_t a, const uint32_t *__restrict__ trace, uint64_t n, uint64_t rows,
                                                                   uint32_t *tab, uint32_t cap, XHelperFlags *fl) {
    const uint64_t t = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x;
    if (t >= rows) return;
    if (!xlookup_insert_lane<NEXT>(XD, a, trace, n, tab, cap, (uint32_t)t, XDevAtomics{})) atomicOr(&fl->exhausted, 1u);
}
template <bool NEXT>
__global__ __launch_bounds__(PERM_BLOCK) void xargs_count_kernel(XArgsDev XD, uint32_t a, const uint32_t *__restrict__ trace, uint64_t n, uint64_t rows,
                                                                  const uint32_t *__restrict__ tab, uint32_t cap, uint32_t *mult, XHelperFlags *fl) {
    const uint64_t r = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x;
    if (r >= rows) return;
    const int got = xlookup_count_lane<NEXT>(XD, a, trace, n, tab, cap, (uint32_t)r, mult, XDevAtomics{});
    if (got == 1) atomicMin(&fl->first, (unsigned long long)r);
    if (got == 2) atomicOr(&fl->exhausted, 1u);
}
// the count launch of a shared lookup: one probe per selected tuple of the lane's row; first: the smallest 4 row + tuple missing
template <bool NEXT>
__global__ __launch_bounds__(PERM_BLOCK) void xargs_count_shared_kernel(XArgsDev XD, XSharedDev SH, uint32_t a, const uint32_t *__restrict__ trace, uint64_t n,
                                                                         uint64_t rows, const uint32_t *__restrict__ tab, uint32_t cap, uint32_t *mult,
                                                                         XHelperFlags *fl) {
    const uint64_t r = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x;
    if (r >= rows) return;
    uint32_t miss = 0;
    const int got = xshared_count_lane<NEXT>(XD, SH, a, trace, n, tab, cap, (uint32_t)r, mult, XDevAtomics{}, &miss);
    if (got & 1) atomicMin(&fl->first, (unsigned long long)(4 * r + miss));
    if (got & 2) atomicOr(&fl->exhausted, 1u);
}

// c: 4 A coordinate columns c_stride apart; block_agg: A runs of nb aggregates (four words each); first: the smallest key
// SHT: XNoShared (xargs_block_kernel) or XSharedDev (xargs_block_shared_kernel, a list with a shared lookup)
// NEXT: the list has a next-row operand.  Such an operand wants the rows row0 + 1 .. row0 + 4, cyclically: three of them are in
// the lane's own 16-byte load, the fourth is one 4-byte load of the word behind it (the neighbour lane's line; word 0 for the
// last lane of the column).  The operand code is wave-uniform, so the whole wave takes the branch.  Without VEC (n < 4, a base
// that is not 16-byte aligned, a stride that is no multiple of 4) and for a periodic column of period 1 or 2 the four cells are
// (row + 1) mod length word by word.  Lists without such an operand take NEXT = false, which is the launch they always took.
template <bool VEC, bool NEXT, class SHT>
__device__ __forceinline__ void xargs_block_body(const XArgsDev &XD, const SHT &SH, const Fp &F, const uint32_t *__restrict__ trace, uint64_t n,
                                                 uint32_t *__restrict__ c, size_t c_stride, uint32_t *__restrict__ block_agg, unsigned long long *first,
                                                 uint32_t (*sc)[4][PERM_BLOCK]) {
    const uint32_t tid = threadIdx.x, a = blockIdx.y;
    const bool perm = XD.kind[a] == SMI_ARG_PERM;
    const uint64_t row0 = ((uint64_t)blockIdx.x * PERM_BLOCK + tid) * PERM_ROWS;
    Fq pl[PERM_ROWS], agg;
    uint64_t key;
    xargs_lane_column(
        XD, SH, a, F, row0, n,
        [&](uint32_t op, uint32_t v[4]) {   // op is wave-uniform
            if (row0 >= n) {
                v[0] = v[1] = v[2] = v[3] = 0u;
            } else if (NEXT && xop_next(op)) {
                const bool per = xop_periodic(op);
                const uint32_t j = op & 0xffu;
                const uint64_t len = per ? 1ull << XD.plog[j] : n, at = row0 & (len - 1);
                const uint32_t *col = per ? XD.pvals + XD.pfirst[j] : trace + (uint64_t)j * n;
                if (VEC && len >= 4) {   // at + 3 < len: the own four are one aligned access, as below
                    uint32_t own[4];
                    perm_load4<true>(col, at, len, own);
                    xargs_next4(col, at, len, own, v);
                } else {
                    xargs_next4_words(col, row0, len, n, v);
                }
            } else if (xop_periodic(op)) {
                const uint32_t j = op & 0xffu, lp = XD.plog[j];
                // P_j >= 4 and row0 a multiple of 4: the four values are consecutive and 16-byte aligned (pfirst[j] is a multiple of P_j)
                if (VEC && lp >= 2) perm_load4<true>(XD.pvals + XD.pfirst[j], row0 & ((1ull << lp) - 1), 1ull << lp, v);
                else xargs_periodic_rows(XD, j, row0, v);
            } else {
                perm_load4<VEC>(trace + (uint64_t)op * n, row0, n, v);
            }
        },
        pl, &agg, &key);
    if (key != ~0ull) atomicMin(first, (unsigned long long)key);
    Fq total;
    const Fq excl = args_wg_scan(perm, agg, sc, tid, XD.g_m, F, &total);
    if (!tid) *(uint4 *)(block_agg + 4 * ((uint64_t)a * gridDim.x + blockIdx.x)) = make_uint4(total.c[0], total.c[1], total.c[2], total.c[3]);
    if (row0 >= n) return;
    uint32_t o[4][PERM_ROWS];
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) {
        const Fq w = args_combine(perm, pl[q], excl, XD.g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) o[e][q] = w.c[e];
    }
    uint32_t *ca = c + 4 * (uint64_t)a * c_stride;
#pragma unroll
    for (int e = 0; e < 4; e++) perm_store4<VEC>(ca + e * c_stride, row0, n, o[e]);
}
template <bool VEC, bool NEXT>
__global__ __launch_bounds__(PERM_BLOCK) void xargs_block_kernel(XArgsDev XD, Fp F, const uint32_t *__restrict__ trace, uint64_t n, uint32_t *__restrict__ c,
                                                                  size_t c_stride, uint32_t *__restrict__ block_agg, unsigned long long *first) {
    __shared__ uint32_t sc[2][4][PERM_BLOCK];
    xargs_block_body<VEC, NEXT>(XD, XNoShared{}, F, trace, n, c, c_stride, block_agg, first, sc);
}
template <bool VEC, bool NEXT>
__global__ __launch_bounds__(PERM_BLOCK) void xargs_block_shared_kernel(XArgsDev XD, XSharedDev SH, Fp F, const uint32_t *__restrict__ trace, uint64_t n,
                                                                         uint32_t *__restrict__ c, size_t c_stride, uint32_t *__restrict__ block_agg,
                                                                         unsigned long long *first) {
    __shared__ uint32_t sc[2][4][PERM_BLOCK];
    xargs_block_body<VEC, NEXT>(XD, SH, F, trace, n, c, c_stride, block_agg, first, sc);
}

// out (four coordinate columns, the composition of the main AIR) += the 2 A auxiliary quotients under w (8 A coordinates).
// plog / pofs / ptab: AirDev's periodic tables on the device.
// NEXT: the list has a next-row operand, f_c(w x) or pi_j(w x): it is read B points further, at i1 -- where the body reads
// the auxiliary columns' next row already.  B, N and every table's length are multiples of 4, so it stays one aligned access.
template <bool VEC, bool NEXT, class SHT>
__device__ __forceinline__ void air_xargs_compose_body(const XArgsDev &XD, const SHT &SH, const Fp &F, uint64_t N, uint32_t log_B, uint32_t h_m, uint32_t omega_m,
                                                       uint32_t tau_m, const uint32_t *__restrict__ izt_m, const uint32_t *__restrict__ plog,
                                                       const uint32_t *__restrict__ pofs, const uint32_t *__restrict__ ptab, const uint32_t *__restrict__ lde,
                                                       size_t stride, const uint32_t *__restrict__ cl, size_t c_stride, const uint64_t *__restrict__ w,
                                                       uint32_t *__restrict__ out, size_t out_stride) {
    const uint64_t groups = N / PERM_ROWS, gid = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x, gstep = (uint64_t)gridDim.x * PERM_BLOCK;
    const uint32_t B = 1u << log_B;
    uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * PERM_ROWS, F), F);
    const uint32_t xstep_m = mont_pow(omega_m, gstep * PERM_ROWS, F);
    for (uint64_t g = gid; g < groups; g += gstep) {
        const uint64_t i0 = g * PERM_ROWS, i1 = (i0 + B) & (N - 1);   // B and N are multiples of 4: no access straddles the wrap
        uint32_t acc[4][PERM_ROWS];
#pragma unroll
        for (int e = 0; e < 4; e++) perm_load4<VEC>(out + e * out_stride, i0, N, acc[e]);
        xargs_compose_points(
            XD, SH, F, w, tau_m, izt_m, B, i0, x_m, omega_m,
            [&](uint32_t op, uint32_t v[4]) {   // op is wave-uniform
                const uint64_t ia = NEXT && xop_next(op) ? i1 : i0;
                if (xop_periodic(op)) {
                    // the table's length L_j = P_j B is a multiple of 4, as i0 is: four consecutive entries, none past the end
                    uint64_t L, at;
                    const uint32_t *table = xargs_table_at(plog, pofs, ptab, op & 0xffu, ia, &L, &at);
                    perm_load4<VEC>(table, at, L, v);
                } else {
                    perm_load4<VEC>(lde + (uint64_t)(NEXT ? op & 0xffu : op) * stride, ia, N, v);
                }
            },
            [&](uint32_t col, bool next, uint32_t v[4]) { perm_load4<VEC>(cl + (uint64_t)col * c_stride, next ? i1 : i0, N, v); }, acc);
#pragma unroll
        for (int e = 0; e < 4; e++) perm_store4<VEC>(out + e * out_stride, i0, N, acc[e]);
        x_m = mont_mul(x_m, xstep_m, F);
    }
}
template <bool VEC, bool NEXT>
__global__ __launch_bounds__(PERM_BLOCK) void air_xargs_compose_kernel(XArgsDev XD, Fp F, uint64_t N, uint32_t log_B, uint32_t h_m, uint32_t omega_m,
                                                                        uint32_t tau_m, const uint32_t *__restrict__ izt_m, const uint32_t *__restrict__ plog,
                                                                        const uint32_t *__restrict__ pofs, const uint32_t *__restrict__ ptab,
                                                                        const uint32_t *__restrict__ lde, size_t stride, const uint32_t *__restrict__ cl,
                                                                        size_t c_stride, const uint64_t *__restrict__ w, uint32_t *__restrict__ out,
                                                                        size_t out_stride) {
    air_xargs_compose_body<VEC, NEXT>(XD, XNoShared{}, F, N, log_B, h_m, omega_m, tau_m, izt_m, plog, pofs, ptab, lde, stride, cl, c_stride, w, out, out_stride);
}
// the sibling a list with a shared lookup takes ("Shared-table lookups"): the tuples travel in SH
template <bool VEC, bool NEXT>
__global__ __launch_bounds__(PERM_BLOCK) void air_xargs_compose_shared_kernel(XArgsDev XD, XSharedDev SH, Fp F, uint64_t N, uint32_t log_B, uint32_t h_m,
                                                                               uint32_t omega_m, uint32_t tau_m, const uint32_t *__restrict__ izt_m,
                                                                               const uint32_t *__restrict__ plog, const uint32_t *__restrict__ pofs,
                                                                               const uint32_t *__restrict__ ptab, const uint32_t *__restrict__ lde, size_t stride,
                                                                               const uint32_t *__restrict__ cl, size_t c_stride, const uint64_t *__restrict__ w,
                                                                               uint32_t *__restrict__ out, size_t out_stride) {
    air_xargs_compose_body<VEC, NEXT>(XD, SH, F, N, log_B, h_m, omega_m, tau_m, izt_m, plog, pofs, ptab, lde, stride, cl, c_stride, w, out, out_stride);
}

namespace {
static_assert(sizeof(XArgsDev) + 160 <= 4096, "the kernel arguments of every launch here stay inside 4 KB");

double xargs_cols_read(const XArgsDev &XD, const XSharedDev *SH) {   // operands read per row, over the arguments
    double cols = SH ? xshared_cols_read(XD, *SH) : 0;
    for (uint32_t a = 0; a < XD.A; a++)
        cols += 2 * XD.m[a] + (XD.kind[a] == SMI_ARG_LOOKUP ? 1 : 0) + (XD.asel[a] != SMI_ARG_NO_SELECTOR) + (XD.bsel[a] != SMI_ARG_NO_SELECTOR);
    return cols;
}
}  // namespace

// bytes of device memory the column build wants: A runs of workgroup aggregates | the flags
size_t xargs_columns_tmp_bytes(uint32_t A, uint64_t n) { return (size_t)A * ((n + PERM_TILE - 1) / PERM_TILE) * 16 + sizeof(ArgsFlags); }
const ArgsFlags *xargs_columns_flags(const uint8_t *d_tmp, uint32_t A, uint64_t n) {
    return (const ArgsFlags *)(d_tmp + (size_t)A * ((n + PERM_TILE - 1) / PERM_TILE) * 16);
}

// the three launches; d_tmp: xargs_columns_tmp_bytes(A, n) bytes, 16-byte aligned; XD.pvals on the device
// SH: the tuples of a list with a shared lookup, which takes the shared instantiation; nullptr for every other list
int xargs_columns_enqueue(smi_ctx *ctx, const XArgsDev &XD, const XSharedDev *SH, const uint32_t *d_trace, uint32_t log_n, uint32_t *d_c, size_t c_stride,
                          uint8_t *d_tmp) {
    const uint64_t n = 1ull << log_n, nb = (n + PERM_TILE - 1) / PERM_TILE;
    uint32_t *d_agg = (uint32_t *)d_tmp;
    ArgsFlags *d_fl = (ArgsFlags *)(d_tmp + (size_t)XD.A * nb * 16);
    const Fp F = ctx->fs.F;
    const bool vec = n >= 4 && al16(d_trace) && al16(d_c) && !(c_stride & 3) && al16(XD.pvals);
    const bool next = xargs_dev_any_next(XD, SH);   // a next-row operand somewhere: the NEXT instantiation
    const dim3 grid((uint32_t)nb, XD.A);
    HIP_TRY(ctx, hipMemsetAsync(&d_fl->first, 0xff, 8, ctx->stream));
    {
        ProfScope ps(ctx, SH ? (next ? "xargs_block_shared_kernel<next>" : "xargs_block_shared_kernel") : next ? "xargs_block_kernel<next>" : "xargs_block_kernel", (4.0 * xargs_cols_read(XD, SH) + 16.0 * XD.A) * (double)n);
        auto shared = vec ? (next ? xargs_block_shared_kernel<true, true> : xargs_block_shared_kernel<true, false>)
                          : (next ? xargs_block_shared_kernel<false, true> : xargs_block_shared_kernel<false, false>);
        auto single = vec ? (next ? xargs_block_kernel<true, true> : xargs_block_kernel<true, false>)
                          : (next ? xargs_block_kernel<false, true> : xargs_block_kernel<false, false>);
        if (SH) shared<<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, *SH, F, d_trace, n, d_c, c_stride, d_agg, &d_fl->first);
        else single<<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, F, d_trace, n, d_c, c_stride, d_agg, &d_fl->first);
        HIP_TRY(ctx, hipGetLastError());
    }
    ArgsScanDev SD{XD.A, XD.g_m, {}};
    for (uint32_t a = 0; a < XD.A; a++) SD.kind[a] = XD.kind[a];
    return args_scan_propagate_enqueue(ctx, SD, n, vec, d_c, c_stride, d_agg, d_fl);
}

// the verdicts of a finished column build (fl: the flags copied to the host).  who, perm_right: how the entry point's
// zero-denominator sentence starts and what it calls a permutation's right side ("xargs_columns", "g_R"; a plain list
// "args_columns", "f_R")
int xargs_columns_verdict(smi_ctx *ctx, const XArgsDev &XD, const XSharedDev *SH, const ArgsFlags &fl, uint32_t *closes, const char *who, const char *perm_right) {
    if (SH && fl.first != ~0ull) {   // the key of a list with a shared lookup: 64 row + 8 a + side, side = j for f_j and J for f_T
        const uint32_t a = (uint32_t)(fl.first >> 3) & 7, side = (uint32_t)fl.first & 7, J = SH->J[a];
        const std::string what = XD.kind[a] == SMI_ARG_PERM ? perm_right : side == J ? "f_T" : J > 1 ? "f_" + std::to_string(side) + " (tuple " + std::to_string(side) + ")" : "f_L";
        const std::string why = std::string(who) + ": argument " + std::to_string(a) + ": " + what + " is zero in row " + std::to_string(fl.first >> 6) + ": no inverse";
        return smi_fail(ctx, SMI_ERR_NO_INVERSE, why.c_str());
    }
    if (fl.first != ~0ull) {
        const uint32_t a = (uint32_t)(fl.first & 15) >> 1;
        const char *side = !(fl.first & 1) ? "f_L" : XD.kind[a] == SMI_ARG_PERM ? perm_right : "f_T";
        const std::string why = std::string(who) + ": argument " + std::to_string(a) + ": " + side + " is zero in row " + std::to_string(fl.first >> 4) + ": no inverse";
        return smi_fail(ctx, SMI_ERR_NO_INVERSE, why.c_str());
    }
    uint32_t mask = 0;
    for (uint32_t a = 0; a < XD.A; a++) {
        const uint32_t *t = fl.total[a];
        if (t[0] == (XD.kind[a] == SMI_ARG_PERM ? 1u : 0u) && !(t[1] | t[2] | t[3])) mask |= 1u << a;
    }
    if (closes) *closes = mask;
    return SMI_OK;
}

// H bound to the device blob and its periodic tables in place (air_periodic_tables, air_compose_ext_launch); d_w: the 8 A
// coordinates behind the main weights
int xargs_compose_enqueue(smi_ctx *ctx, const XArgsDev &XD, const XSharedDev *SH, const AirHost &H, uint32_t tau, const uint32_t *d_lde, size_t stride, const uint32_t *d_cl,
                          size_t c_stride, const uint64_t *d_w, uint32_t *d_out, size_t out_stride) {
    const AirDev &A = H.dev;
    const Fp F = ctx->fs.F;
    // the periodic loader rests on this: every table's length P_j B is a multiple of 4 and every table starts at a multiple of
    // its length (air_periodic_plan), so four entries from a multiple of 4 are consecutive, aligned and inside the table
    if (A.log_B < 2) return smi_fail(ctx, SMI_ERR_EXPANSION_TOO_SMALL, "air_compose_xargs: log_blowup < 2");
    for (uint32_t j = 0; j < A.Q; j++)
        if (H.per.ofs[j] & ((1u << H.per.log_len[j]) - 1u)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_xargs: a periodic table does not start at a multiple of its length");
    const bool vec = al16(d_lde) && al16(d_cl) && al16(d_out) && !(stride & 3) && !(c_stride & 3) && !(out_stride & 3) && (!A.Q || al16(A.ptab));
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK, cap = (uint64_t)ctx->num_cus * 8;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint32_t tau_m = air_to_m(tau, F.p);
    const bool next = xargs_dev_any_next(XD, SH);   // a next-row operand somewhere: the NEXT instantiation
    ProfScope ps(ctx, SH ? (next ? "air_xargs_compose_shared_kernel<next>" : "air_xargs_compose_shared_kernel") : next ? "air_xargs_compose_kernel<next>" : "air_xargs_compose_kernel",
                 (4.0 * xargs_cols_read(XD, SH) + 32.0 * XD.A + 32.0) * (double)A.N);
    auto shared = vec ? (next ? air_xargs_compose_shared_kernel<true, true> : air_xargs_compose_shared_kernel<true, false>)
                      : (next ? air_xargs_compose_shared_kernel<false, true> : air_xargs_compose_shared_kernel<false, false>);
    auto single = vec ? (next ? air_xargs_compose_kernel<true, true> : air_xargs_compose_kernel<true, false>)
                      : (next ? air_xargs_compose_kernel<false, true> : air_xargs_compose_kernel<false, false>);
    if (SH)
        shared<<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, *SH, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, A.izt_m, A.plog, A.pofs, A.ptab, d_lde, stride, d_cl, c_stride, d_w,
                                                     d_out, out_stride);
    else
        single<<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, A.izt_m, A.plog, A.pofs, A.ptab, d_lde, stride, d_cl, c_stride, d_w, d_out,
                                                     out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

// the checks every entry point without a cfg starts with
int xargs_args(smi_ctx *ctx, const smi_air *air, const smi_air_xargs *xargs, uint32_t n_cols, uint32_t log_n) {
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "xargs: modulus must be < 2^30");
    std::string why;
    if (!n_cols || n_cols > 64) return smi_fail(ctx, SMI_ERR_BAD_ARG, "xargs: 1..64 columns");
    if (log_n < 1 || log_n > 27) return smi_fail(ctx, SMI_ERR_BAD_ARG, "xargs: log_n must be in 1 .. 27");
    const int prc = xargs_periodic_check(ctx->fs.F.p, air, log_n, &why);
    if (prc != SMI_OK) return smi_fail(ctx, prc, why.c_str());
    if (xargs_validate(xargs, n_cols, air->n_periodic, &why) != SMI_OK) return smi_fail(ctx, SMI_ERR_BAD_ARG, why.c_str());
    if (xargs_shared_rows(ctx->fs.F.p, xargs, log_n, &why) != SMI_OK) return smi_fail(ctx, SMI_ERR_BAD_ARG, why.c_str());
    return SMI_OK;
}

// the helper over the first `rows` rows: table rows at and above `rows` are not inserted, lookup rows there are not counted;
// all n words of d_mult are written (zero where nothing is counted).  bounded: the caller is the entry point with a row bound,
// which takes this-row operands only (what lies behind the bound is not the caller's successor row)
static int xargs_multiplicities_run(smi_ctx *ctx, const void *air_, const void *xargs_, uint32_t a, const uint32_t *d_trace_cols, uint32_t n_cols,
                                    uint32_t log_n, size_t rows, uint32_t *d_mult, bool bounded) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_xargs *xargs = (const smi_air_xargs *)xargs_;
    if (!ctx || !air || !xargs || !d_trace_cols || !d_mult) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(xargs_args(ctx, air, xargs, n_cols, log_n));
    if (bounded) {
        std::string why;
        if (xargs_refuse_next(xargs, "xargs_multiplicities_rows", "the helper over a row bound takes this-row operands only", &why) != SMI_OK)
            return smi_fail(ctx, SMI_ERR_BAD_ARG, why.c_str());
    }
    if (a >= xargs->count) return smi_fail(ctx, SMI_ERR_BAD_ARG, "xargs_multiplicities: no such argument");
    if ((xargs->arg[a].kind & 0xffu) != SMI_ARG_LOOKUP) {
        const std::string why = "xargs_multiplicities: argument " + std::to_string(a) + " is a permutation: it has no multiplicities";
        return smi_fail(ctx, SMI_ERR_BAD_ARG, why.c_str());
    }
    const uint64_t n = 1ull << log_n, cap = lookup_table_slots(n);
    if (!rows || rows > n) return smi_fail(ctx, SMI_ERR_BAD_ARG, "xargs_multiplicities_rows: rows must be in 1 .. n");
    AirPeriodic per;
    xargs_periodic_plan(ctx->fs.F.p, air, log_n, &per);
    XArgsDev XD;
    const uint64_t no_challenges[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the helper reads the operand lists alone
    xargs_build(ctx->fs.F, ctx->fs.g, xargs, n_cols, air, per, no_challenges, &XD);
    XSharedDev SH;
    xshared_build(xargs, n_cols, &SH);
    const uint32_t J = SH.J[a];
    void *tmp = nullptr;   // the table | the flags | the periodic values
    SMI_TRY(ctx_tmp(ctx, 3, cap * 4 + sizeof(XHelperFlags) + per.vals.size() * 4, &tmp));
    uint32_t *d_tab = (uint32_t *)tmp;
    XHelperFlags *d_fl = (XHelperFlags *)((uint8_t *)tmp + cap * 4);
    uint32_t *d_pvals = (uint32_t *)((uint8_t *)tmp + cap * 4 + sizeof(XHelperFlags));
    XD.pvals = d_pvals;
    HIP_TRY(ctx, hipMemsetAsync(d_tab, 0xff, cap * 4 + 8, ctx->stream));   // every slot free; no row missing yet
    HIP_TRY(ctx, hipMemsetAsync(&d_fl->exhausted, 0, 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_mult, 0, n * 4, ctx->stream));
    if (!per.vals.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_pvals, per.vals.data(), per.vals.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t grid = (uint32_t)((rows + PERM_BLOCK - 1) / PERM_BLOCK), m = XD.m[a];
    const bool next = xargs_dev_any_next(XD, &SH);   // a next-row operand somewhere in the list: the NEXT instantiations
    {
        ProfScope ps(ctx, "xargs_insert_kernel", (4.0 * m + 4.0) * (double)n);
        (next ? xargs_insert_kernel<true> : xargs_insert_kernel<false>)<<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, a, d_trace_cols, n, rows, d_tab, (uint32_t)cap, d_fl);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, J > 1 ? "xargs_count_shared_kernel" : "xargs_count_kernel", (4.0 * 2 * m + 8.0) * J * (double)n);
        if (J > 1)
            (next ? xargs_count_shared_kernel<true> : xargs_count_shared_kernel<false>)<<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, SH, a, d_trace_cols, n, rows, d_tab,
                                                                                                                              (uint32_t)cap, d_mult, d_fl);
        else
            (next ? xargs_count_kernel<true> : xargs_count_kernel<false>)<<<grid, PERM_BLOCK, 0, ctx->stream>>>(XD, a, d_trace_cols, n, rows, d_tab, (uint32_t)cap, d_mult, d_fl);
        HIP_TRY(ctx, hipGetLastError());
    }
    XHelperFlags fl;
    HIP_TRY(ctx, hipMemcpyAsync(&fl, d_fl, sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // per.vals has been read by now
    if (fl.exhausted) return smi_fail(ctx, SMI_ERR_BAD_ARG, "xargs_multiplicities: a probe ran through the whole table");
    if (fl.first != ~0ull && J > 1) {   // 4 row + tuple
        const std::string why = "xargs_multiplicities: argument " + std::to_string(a) + ": tuple " + std::to_string(fl.first & 3) + " of row " +
                                std::to_string(fl.first >> 2) + ", which its selector selects, is in no selected table row";
        return smi_fail(ctx, SMI_ERR_LOOKUP_MISSING, why.c_str());
    }
    if (fl.first != ~0ull) {
        const std::string why = "xargs_multiplicities: argument " + std::to_string(a) + ": the tuple of selected row " + std::to_string(fl.first) +
                                " is in no selected table row";
        return smi_fail(ctx, SMI_ERR_LOOKUP_MISSING, why.c_str());
    }
    return SMI_OK;
}
int smi_dev_xargs_multiplicities(smi_ctx *ctx, const void *air_, const void *xargs_, uint32_t a, const uint32_t *d_trace_cols, uint32_t n_cols,
                                 uint32_t log_n, uint32_t *d_mult) {
    return xargs_multiplicities_run(ctx, air_, xargs_, a, d_trace_cols, n_cols, log_n, (size_t)1 << (log_n < 63 ? log_n : 0), d_mult, false);
}
int smi_dev_xargs_multiplicities_rows(smi_ctx *ctx, const void *air_, const void *xargs_, uint32_t a, const uint32_t *d_trace_cols, uint32_t n_cols,
                                      uint32_t log_n, size_t rows, uint32_t *d_mult) {
    return xargs_multiplicities_run(ctx, air_, xargs_, a, d_trace_cols, n_cols, log_n, rows, d_mult, true);
}

// ---- what the entry points of both lists run behind their checks (the plain list's are in args.hip).  air: the AIR whose
// periodic columns the operands may name; nullptr for a plain list, which has no periodic operand: its tables are built
// without a look at them, and the periodic values the kernels are handed stay unread.  nm: the entry points' own words.
int xargs_columns_run(smi_ctx *ctx, const smi_air *air, const smi_air_xargs *xargs, const ListNames &nm, const uint32_t *d_trace_cols, uint32_t n_cols,
                      uint32_t log_n, const uint64_t *challenges, uint32_t *d_c, size_t c_stride, uint32_t *closes) {
    const uint64_t n = 1ull << log_n;
    AirPeriodic per;
    if (air) xargs_periodic_plan(ctx->fs.F.p, air, log_n, &per);
    XArgsDev XD;
    xargs_build(ctx->fs.F, ctx->fs.g, xargs, n_cols, air, per, challenges, &XD);
    XSharedDev SHs;
    const XSharedDev *SH = xshared_build(xargs, n_cols, &SHs) ? &SHs : nullptr;
    const size_t b_tmp = up16(xargs_columns_tmp_bytes(XD.A, n));
    void *tmp = nullptr;   // the aggregates and flags | the periodic values
    SMI_TRY(ctx_tmp(ctx, 3, b_tmp + per.vals.size() * 4, &tmp));
    uint32_t *d_pvals = (uint32_t *)((uint8_t *)tmp + b_tmp);
    XD.pvals = d_pvals;
    if (!per.vals.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_pvals, per.vals.data(), per.vals.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SMI_TRY(xargs_columns_enqueue(ctx, XD, SH, d_trace_cols, log_n, d_c, c_stride, (uint8_t *)tmp));
    ArgsFlags fl;
    HIP_TRY(ctx, hipMemcpyAsync(&fl, xargs_columns_flags((const uint8_t *)tmp, XD.A, n), sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return xargs_columns_verdict(ctx, XD, SH, fl, closes, nm.columns, nm.perm_right);
}

// H: air_host_tables of the proof's AIR -- its periodic tables are built for the main composition whatever the list reads
int xargs_compose_run(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, const smi_air *air, const smi_air_xargs *xargs, const uint32_t *d_lde, size_t stride,
                      const uint32_t *d_c_lde, size_t c_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out, size_t out_stride) {
    const size_t b_tab = up16(H.per.table_words * 4), b_vals = up16(H.per.vals.size() * 4);
    void *base = nullptr;   // tables | grouped values | blob
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_vals + H.blob.size() * 4, &base));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, (uint32_t *)((uint8_t *)base + b_tab), (uint32_t *)base));
    SMI_TRY(air_compose_ext_launch(ctx, H, (uint32_t *)((uint8_t *)base + b_tab + b_vals), d_lde, stride, d_weights, d_out, out_stride));
    XArgsDev XD;
    xargs_build(ctx->fs.F, ctx->fs.g, xargs, cfg->n_cols, air, air ? H.per : AirPeriodic{}, challenges, &XD);
    XSharedDev SHs;
    const XSharedDev *SH = xshared_build(xargs, cfg->n_cols, &SHs) ? &SHs : nullptr;
    return xargs_compose_enqueue(ctx, XD, SH, H, (uint32_t)cfg->trace_offset, d_lde, stride, d_c_lde, c_stride, d_weights + 4 * (size_t)(cfg->n_cols + H.dev.K), d_out,
                                 out_stride);
}

// the list as a variant of the two-tree prover (internal.h): one auxiliary column per argument
int xargs_prove_run(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, uint64_t E, const smi_air *air, const smi_air_xargs *xargs, const ListNames &nm,
                    const uint32_t *d_trace_cols, uint8_t *roots_out, uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms,
                    uint32_t grind_bits, uint32_t *closes) {
    const uint32_t W = cfg->n_cols, A = xargs->count;
    const size_t n = (size_t)1 << cfg->log_n, N = n << cfg->log_blowup;
    XArgsDev XD;
    XSharedDev SHs;
    const XSharedDev *SH = nullptr;
    TwoTreeVariant v;
    v.name = nm.prove;
    v.A = A;
    v.tmp_bytes = xargs_columns_tmp_bytes(A, n);
    v.flags_bytes = sizeof(ArgsFlags);
    v.columns = [&](const uint64_t *ch, const uint32_t *d_pvals, uint32_t *d_c, uint8_t *d_tmp) {
        xargs_build(ctx->fs.F, ctx->fs.g, xargs, W, air, air ? H.per : AirPeriodic{}, ch, &XD);
        XD.pvals = air ? d_pvals : nullptr;   // the raw values the column build reads
        SH = xshared_build(xargs, W, &SHs) ? &SHs : nullptr;
        return xargs_columns_enqueue(ctx, XD, SH, d_trace_cols, cfg->log_n, d_c, n, d_tmp);
    };
    v.settle = [&](const void *fl) { return xargs_columns_verdict(ctx, XD, SH, *(const ArgsFlags *)fl, closes, nm.columns, nm.perm_right); };
    v.compose = [&](const AirHost &Hd, const uint32_t *d_lde, const uint32_t *d_cl, const uint64_t *d_w, uint32_t *d_cw) {
        return xargs_compose_enqueue(ctx, XD, SH, Hd, (uint32_t)cfg->trace_offset, d_lde, N, d_cl, N, d_w, d_cw, N);
    };
    return two_tree_prove(ctx, cfg, H, E, d_trace_cols, v, roots_out, proof, proof_len, top_indices, stage_ms, grind_bits);
}

static const ListNames XARGS_NAMES = {"xargs_columns", "g_R", "air_prove_xargs"};

int smi_dev_xargs_columns(smi_ctx *ctx, const void *air_, const void *xargs_, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n,
                          const uint64_t *challenges, uint32_t *d_c, size_t c_stride, uint32_t *closes) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_xargs *xargs = (const smi_air_xargs *)xargs_;
    if (!ctx || !air || !xargs || !d_trace_cols || !challenges || !d_c) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(xargs_args(ctx, air, xargs, n_cols, log_n));
    if (c_stride < (1ull << log_n)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "xargs_columns: c_stride < n");
    return xargs_columns_run(ctx, air, xargs, XARGS_NAMES, d_trace_cols, n_cols, log_n, challenges, d_c, c_stride, closes);
}

int smi_dev_air_compose_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const void *xargs_, const uint32_t *d_lde, size_t stride,
                              const uint32_t *d_c_lde, size_t c_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                              size_t out_stride) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_xargs *xargs = (const smi_air_xargs *)xargs_;
    if (!ctx || !cfg || !air || !xargs || !d_lde || !d_c_lde || !challenges || !d_weights || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    AirHost H;
    SMI_TRY(air_host_tables(ctx, cfg, air, &H, nullptr));
    SMI_TRY(xargs_args(ctx, air, xargs, cfg->n_cols, cfg->log_n));
    if (stride < H.dev.N || out_stride < H.dev.N || c_stride < H.dev.N)
        return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_xargs: stride < N, c_stride < N or out_stride < N");
    return xargs_compose_run(ctx, cfg, H, air, xargs, d_lde, stride, d_c_lde, c_stride, challenges, d_weights, d_out, out_stride);
}

int smi_dev_air_prove_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const void *xargs_, const uint32_t *d_trace_cols, uint8_t *roots_out,
                            uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, uint32_t *closes) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_xargs *xargs = (const smi_air_xargs *)xargs_;
    if (!ctx || !cfg || !air || !xargs || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    AirHost H;
    uint64_t E = 0;
    SMI_TRY(air_host_tables(ctx, cfg, air, &H, &E));   // E of the AIR alone; the plan below counts the auxiliary transitions in
    SMI_TRY(xargs_args(ctx, air, xargs, cfg->n_cols, cfg->log_n));
    {
        std::string why;
        const int rc = xargs_plan(ctx->fs.F.p, cfg, air, xargs, nullptr, &E, &why);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    return xargs_prove_run(ctx, cfg, H, E, air, xargs, XARGS_NAMES, d_trace_cols, roots_out, proof, proof_len, top_indices, stage_ms, grind_bits, closes);
}
