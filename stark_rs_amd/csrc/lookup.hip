// lookup.hip -- the LogUp lookup argument over a committed extension column (include/stark_mi.h, "Lookup argument"): the
// multiplicity helper, the column s by batched F_q division and a device-wide prefix sum, the two auxiliary quotients added
// into the composition codeword, and the prover with its second commitment round.  The lane bodies are lookup_core.h,
// shared with the CPU emulator (emu_lookup.cpp); the verifier is in verify.hip.  The construction is perm.hip's with a sum
// where that has a product.
//
// The helper is two launches over an open-addressing table of row indices (2 n slots, preset to all-ones):
//   lookup_insert_kernel   lane t claims the first free slot of its table tuple's probe sequence, or lowers the row a slot
//                          of the same tuple holds (atomicCAS / atomicMin);
//   lookup_count_kernel    lane r probes for its lookup tuple and adds one to the multiplicity of the row it finds; the lanes
//                          of a wave that find the same row in the same trip send one atomic between them.
// Every probe loop is bounded by the table's size; no lane waits on another.
//
// The column build is the multi-launch scan of perm.hip:
//   lookup_block_kernel      a lane takes PERM_ROWS consecutive rows, forms f_L, f_T and M, inverts its four products f_L f_T
//                            with one F_q inversion and sums up its delta; the workgroup scans the lane sums in LDS; every
//                            row gets its prefix WITHIN the workgroup (stored to s, plain) and the workgroup its sum;
//   lookup_scan_kernel       one workgroup loops over the workgroup sums, PERM_BLOCK at a time, and leaves exclusive
//                            prefixes in their place, and the total;
//   lookup_propagate_kernel  s[r] += prefix of r's workgroup: four additions per row.
//
// air_lookup_compose_kernel streams as air_perm_compose_kernel does, with one more column (M) read per point.
#include <string>
#include <vector>

#include "air_core.h"
#include "hash_core.h"
#include "internal.h"
#include "lookup_core.h"
#include "mgpu_core.h"
#include "row4_dev.h"

namespace {
struct DevAtomics {
    __device__ __forceinline__ uint32_t cas(uint32_t *a, uint32_t expect, uint32_t v) const { return atomicCAS(a, expect, v); }
    __device__ __forceinline__ void min(uint32_t *a, uint32_t v) const { atomicMin(a, v); }
    // Lanes of a wave that arrive here together and count into the same word send ONE atomic with their sum: equal lookup
    // tuples walk the same probe sequence, so they arrive in the same trip of the probe loop, and a table entry that a whole
    // wave hits would otherwise take 64 atomics on one address one after the other.  Each trip retires the first lane still
    // here and every lane with its address: at most 64 trips, and no lane waits for a lane that is not in the trip.
    __device__ __forceinline__ void add(uint32_t *a, uint32_t v) const {
        const uint64_t mine = (uint64_t)(uintptr_t)a;
        for (int trip = 0; trip < 64; trip++) {
            const uint32_t lead_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(mine >> 32)), lead_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)mine);
            const uint64_t lead = ((uint64_t)lead_hi << 32) | lead_lo;   // the builtin returns int: no sign extension into the high word
            const uint64_t peers = __ballot(mine == lead);
            if (mine == lead) {
                if ((uint32_t)__lane_id() == (uint32_t)__ffsll((long long)peers) - 1) atomicAdd(a, v * (uint32_t)__popcll(peers));
                return;
            }
        }
    }
};
struct HelperFlags {   // as the helper leaves them on the device: the first missing row, a probe that ran out
    unsigned long long first;
    uint32_t exhausted, pad;
};

// the workgroup scan of lookup_core.h (lookup_scan_step) between barriers; returns the lane's EXCLUSIVE prefix and the
// workgroup's sum.  sc: 2 x 4 x PERM_BLOCK words of LDS.
__device__ __forceinline__ Fq lookup_wg_scan(Fq v, uint32_t (*sc)[4][PERM_BLOCK], uint32_t tid, uint32_t p, Fq *total) {
    __syncthreads();   // the buffers of the scan before are consumed
#pragma unroll
    for (int e = 0; e < 4; e++) sc[0][e][tid] = v.c[e];
    __syncthreads();
    int cur = 0;
    for (uint32_t off = 1; off < PERM_BLOCK; off <<= 1) {
        lookup_scan_step(sc[cur], sc[cur ^ 1], tid, off, p);
        __syncthreads();
        cur ^= 1;
    }
    *total = perm_scan_at(sc[cur], PERM_BLOCK - 1);
    return tid ? perm_scan_at(sc[cur], tid - 1) : Fq{{0, 0, 0, 0}};
}
}  // namespace

__global__ __launch_bounds__(PERM_BLOCK) void lookup_insert_kernel(LookupDev LD, const uint32_t *__restrict__ trace, uint64_t n, uint32_t *tab, uint32_t cap,
                                                                    HelperFlags *fl) {
    const uint64_t t = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x;
    if (t >= n) return;
    if (!lookup_insert_lane(LD, trace, n, tab, cap, (uint32_t)t, DevAtomics{})) atomicOr(&fl->exhausted, 1u);
}
__global__ __launch_bounds__(PERM_BLOCK) void lookup_count_kernel(LookupDev LD, const uint32_t *__restrict__ trace, uint64_t n, const uint32_t *__restrict__ tab,
                                                                   uint32_t cap, uint32_t *mult, HelperFlags *fl) {
    const uint64_t r = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x;
    if (r >= n) return;
    const int got = lookup_count_lane(LD, trace, n, tab, cap, (uint32_t)r, mult, DevAtomics{});
    if (got == 1) atomicMin(&fl->first, (unsigned long long)r);
    if (got == 2) atomicOr(&fl->exhausted, 1u);
}

template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void lookup_block_kernel(LookupDev LD, Fp F, const uint32_t *__restrict__ trace, uint64_t n, uint32_t *__restrict__ s,
                                                                   size_t s_stride, uint32_t *__restrict__ block_sum, unsigned long long *first) {
    __shared__ uint32_t sc[2][4][PERM_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint64_t row0 = ((uint64_t)blockIdx.x * PERM_BLOCK + tid) * PERM_ROWS;
    Fq sl[PERM_ROWS], sum;
    uint64_t zero_at;
    lookup_lane_column(
        LD, F, row0, n,
        [&](uint32_t col, uint32_t v[4]) {
            if (row0 < n) perm_load4<VEC>(trace + (uint64_t)col * n, row0, n, v);
            else v[0] = v[1] = v[2] = v[3] = 0u;
        },
        sl, &sum, &zero_at);
    if (zero_at != ~0ull) atomicMin(first, (unsigned long long)zero_at);
    Fq total;
    const Fq excl = lookup_wg_scan(sum, sc, tid, F.p, &total);
    if (!tid) *(uint4 *)(block_sum + 4 * (uint64_t)blockIdx.x) = make_uint4(total.c[0], total.c[1], total.c[2], total.c[3]);
    if (row0 >= n) return;
    uint32_t o[4][PERM_ROWS];
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) {
        const Fq w = fq_add(sl[q], excl, F.p);
#pragma unroll
        for (int e = 0; e < 4; e++) o[e][q] = w.c[e];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) perm_store4<VEC>(s + e * s_stride, row0, n, o[e]);
}

// bs: nb workgroup sums (four words each) -> their exclusive prefixes; total: the sum of all
__global__ __launch_bounds__(PERM_BLOCK) void lookup_scan_kernel(uint32_t p, uint32_t nb, uint32_t *__restrict__ bs, uint32_t *__restrict__ total) {
    __shared__ uint32_t sc[2][4][PERM_BLOCK];
    const uint32_t tid = threadIdx.x;
    Fq carry{{0, 0, 0, 0}};
    for (uint32_t base = 0; base < nb; base += PERM_BLOCK) {   // wave-uniform trip count
        const bool in = base + tid < nb;
        Fq v{{0, 0, 0, 0}};
        if (in) {
            const uint4 t = *(const uint4 *)(bs + 4 * (uint64_t)(base + tid));
            v = Fq{{t.x, t.y, t.z, t.w}};
        }
        Fq tile;
        const Fq excl = lookup_wg_scan(v, sc, tid, p, &tile);
        if (in) {
            const Fq w = fq_add(carry, excl, p);
            *(uint4 *)(bs + 4 * (uint64_t)(base + tid)) = make_uint4(w.c[0], w.c[1], w.c[2], w.c[3]);
        }
        carry = fq_add(carry, tile, p);
    }
    if (!tid) *(uint4 *)total = make_uint4(carry.c[0], carry.c[1], carry.c[2], carry.c[3]);
}

template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void lookup_propagate_kernel(uint32_t p, uint64_t n, uint32_t *__restrict__ s, size_t s_stride,
                                                                       const uint32_t *__restrict__ block_excl) {
    const uint64_t row0 = ((uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x) * PERM_ROWS;
    if (row0 >= n) return;
    const uint4 t = *(const uint4 *)(block_excl + 4 * (uint64_t)blockIdx.x);   // wave-uniform
    const uint32_t pre[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        uint32_t v[PERM_ROWS];
        perm_load4<VEC>(s + e * s_stride, row0, n, v);
#pragma unroll
        for (int q = 0; q < PERM_ROWS; q++) v[q] = fp_add(v[q], pre[e], p);
        perm_store4<VEC>(s + e * s_stride, row0, n, v);
    }
}

// out (four coordinate columns, the composition of the main AIR) += w_b * boundary quotient + w_t * transition quotient of s
template <bool VEC>
__global__ __launch_bounds__(PERM_BLOCK) void air_lookup_compose_kernel(LookupDev LD, Fp F, uint64_t N, uint32_t log_B, uint32_t h_m, uint32_t omega_m,
                                                                         uint32_t tau_m, const uint32_t *__restrict__ izt_m, const uint32_t *__restrict__ lde,
                                                                         size_t stride, const uint32_t *__restrict__ sl, size_t s_stride,
                                                                         const uint64_t *__restrict__ w, uint32_t *__restrict__ out, size_t out_stride) {
    uint32_t wm[4];
#pragma unroll
    for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[e], F);
    const ExtMul wb = ext_mul_prepare(wm, LD.P.g_m, F);
#pragma unroll
    for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[4 + e], F);
    const ExtMul wt = ext_mul_prepare(wm, LD.P.g_m, F);
    const uint64_t groups = N / PERM_ROWS, gid = (uint64_t)blockIdx.x * PERM_BLOCK + threadIdx.x, gstep = (uint64_t)gridDim.x * PERM_BLOCK;
    const uint32_t B = 1u << log_B;
    uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * PERM_ROWS, F), F);
    const uint32_t xstep_m = mont_pow(omega_m, gstep * PERM_ROWS, F);
    for (uint64_t g = gid; g < groups; g += gstep) {
        const uint64_t i0 = g * PERM_ROWS, i1 = (i0 + B) & (N - 1);   // B and N are multiples of 4: no access straddles the wrap
        uint32_t sc[4][PERM_ROWS], sx[4][PERM_ROWS], acc[4][PERM_ROWS];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            perm_load4<VEC>(sl + e * s_stride, i0, N, sc[e]);
            perm_load4<VEC>(sl + e * s_stride, i1, N, sx[e]);
            perm_load4<VEC>(out + e * out_stride, i0, N, acc[e]);
        }
        lookup_compose_points(
            LD, F, wb, wt, tau_m, izt_m, B, i0, x_m, omega_m, [&](uint32_t col, uint32_t v[4]) { perm_load4<VEC>(lde + (uint64_t)col * stride, i0, N, v); }, sc, sx,
            acc);
#pragma unroll
        for (int e = 0; e < 4; e++) perm_store4<VEC>(out + e * out_stride, i0, N, acc[e]);
        x_m = mont_mul(x_m, xstep_m, F);
    }
}

namespace {
// bytes of device scratch the column build wants: the workgroup sums | the total (16) | the first zero (8, padded)
size_t lookup_column_tmp_bytes(uint64_t n) { return ((n + PERM_TILE - 1) / PERM_TILE) * 16 + 32; }

struct LookupFlags {   // as the column build leaves them on the device: total (4 words), first zero as 2 row + (f_T ? 1 : 0)
    uint32_t total[4];
    unsigned long long first;
    unsigned long long pad;
};

// the three launches; d_tmp: lookup_column_tmp_bytes(n) bytes, 16-byte aligned.  The flags are at d_tmp + nb * 16.
int lookup_column_enqueue(smi_ctx *ctx, const LookupDev &LD, const uint32_t *d_trace, uint32_t log_n, uint32_t *d_s, size_t s_stride, uint8_t *d_tmp) {
    const uint64_t n = 1ull << log_n, nb = (n + PERM_TILE - 1) / PERM_TILE;
    uint32_t *d_bs = (uint32_t *)d_tmp;
    LookupFlags *d_fl = (LookupFlags *)(d_tmp + nb * 16);
    const Fp F = ctx->fs.F;
    const bool vec = n >= 4 && al16(d_trace) && al16(d_s) && !(s_stride & 3);
    HIP_TRY(ctx, hipMemsetAsync(&d_fl->first, 0xff, 8, ctx->stream));
    {
        ProfScope ps(ctx, "lookup_block_kernel", (4.0 * (2 * LD.P.m + 1) + 16.0) * (double)n);
        if (vec) lookup_block_kernel<true><<<(uint32_t)nb, PERM_BLOCK, 0, ctx->stream>>>(LD, F, d_trace, n, d_s, s_stride, d_bs, &d_fl->first);
        else lookup_block_kernel<false><<<(uint32_t)nb, PERM_BLOCK, 0, ctx->stream>>>(LD, F, d_trace, n, d_s, s_stride, d_bs, &d_fl->first);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, "lookup_scan_kernel", 32.0 * (double)nb);
        lookup_scan_kernel<<<1, PERM_BLOCK, 0, ctx->stream>>>(F.p, (uint32_t)nb, d_bs, d_fl->total);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, "lookup_propagate_kernel", 32.0 * (double)n);
        if (vec) lookup_propagate_kernel<true><<<(uint32_t)nb, PERM_BLOCK, 0, ctx->stream>>>(F.p, n, d_s, s_stride, d_bs);
        else lookup_propagate_kernel<false><<<(uint32_t)nb, PERM_BLOCK, 0, ctx->stream>>>(F.p, n, d_s, s_stride, d_bs);
        HIP_TRY(ctx, hipGetLastError());
    }
    return SMI_OK;
}
const LookupFlags *lookup_column_flags(const uint8_t *d_tmp, uint32_t log_n) {
    return (const LookupFlags *)(d_tmp + (((1ull << log_n) + PERM_TILE - 1) / PERM_TILE) * 16);
}

// the verdicts of a finished column build (fl: the flags copied to the host)
int lookup_column_verdict(smi_ctx *ctx, const LookupFlags &fl, int *closes) {
    if (fl.first != ~0ull) {
        const std::string why = std::string("lookup_column: ") + ((fl.first & 1) ? "f_T" : "f_L") + " is zero in row " + std::to_string(fl.first >> 1) + ": no inverse";
        return smi_fail(ctx, SMI_ERR_NO_INVERSE, why.c_str());
    }
    if (closes) *closes = !(fl.total[0] | fl.total[1] | fl.total[2] | fl.total[3]);
    return SMI_OK;
}

// H bound to the device blob (air_compose_ext_launch leaves it so)
int lookup_compose_enqueue(smi_ctx *ctx, const LookupDev &LD, const AirHost &H, uint32_t tau, const uint32_t *d_lde, size_t stride, const uint32_t *d_sl,
                           size_t s_stride, const uint64_t *d_w8, uint32_t *d_out, size_t out_stride) {
    const AirDev &A = H.dev;
    const Fp F = ctx->fs.F;
    const bool vec = al16(d_lde) && al16(d_sl) && al16(d_out) && !(stride & 3) && !(s_stride & 3) && !(out_stride & 3);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK, cap = (uint64_t)ctx->num_cus * 8;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint32_t tau_m = air_to_m(tau, F.p);
    ProfScope ps(ctx, "air_lookup_compose_kernel", (4.0 * (2 * LD.P.m + 1) + 32.0 + 32.0) * (double)A.N);
    if (vec)
        air_lookup_compose_kernel<true><<<grid, PERM_BLOCK, 0, ctx->stream>>>(LD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, A.izt_m, d_lde, stride, d_sl, s_stride,
                                                                              d_w8, d_out, out_stride);
    else
        air_lookup_compose_kernel<false><<<grid, PERM_BLOCK, 0, ctx->stream>>>(LD, F, A.N, A.log_B, A.h_m, A.omega_m, tau_m, A.izt_m, d_lde, stride, d_sl, s_stride,
                                                                               d_w8, d_out, out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int lookup_args(smi_ctx *ctx, const smi_air_lookup *lk, uint32_t n_cols, uint32_t log_n) {
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "lookup: modulus must be < 2^30");
    std::string why;
    if (!n_cols || n_cols > 64) return smi_fail(ctx, SMI_ERR_BAD_ARG, "lookup: 1..64 columns");
    if (log_n < 1 || log_n > 27) return smi_fail(ctx, SMI_ERR_BAD_ARG, "lookup: log_n must be in 1 .. 27");
    if (lookup_validate(lk, n_cols, &why) != SMI_OK) return smi_fail(ctx, SMI_ERR_BAD_ARG, why.c_str());
    return SMI_OK;
}
}  // namespace

int smi_dev_lookup_multiplicities(smi_ctx *ctx, const void *lookup_, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, uint32_t *d_mult) {
    const smi_air_lookup *lk = (const smi_air_lookup *)lookup_;
    if (!ctx || !lk || !d_trace_cols || !d_mult) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(lookup_args(ctx, lk, n_cols, log_n));
    const uint64_t n = 1ull << log_n, cap = lookup_table_slots(n);
    LookupDev LD;
    const uint64_t no_challenges[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the helper reads the column lists alone
    lookup_build(ctx->fs.F, ctx->fs.g, lk, no_challenges, &LD);
    void *tmp = nullptr;   // the table | the flags
    SMI_TRY(ctx_tmp(ctx, 3, cap * 4 + sizeof(HelperFlags), &tmp));
    uint32_t *d_tab = (uint32_t *)tmp;
    HelperFlags *d_fl = (HelperFlags *)((uint8_t *)tmp + cap * 4);
    HIP_TRY(ctx, hipMemsetAsync(d_tab, 0xff, cap * 4 + 8, ctx->stream));   // every slot free; no row missing yet
    HIP_TRY(ctx, hipMemsetAsync(&d_fl->exhausted, 0, 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_mult, 0, n * 4, ctx->stream));
    const uint32_t grid = (uint32_t)((n + PERM_BLOCK - 1) / PERM_BLOCK);
    {
        ProfScope ps(ctx, "lookup_insert_kernel", (4.0 * LD.P.m + 4.0) * (double)n);
        lookup_insert_kernel<<<grid, PERM_BLOCK, 0, ctx->stream>>>(LD, d_trace_cols, n, d_tab, (uint32_t)cap, d_fl);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, "lookup_count_kernel", (4.0 * 2 * LD.P.m + 8.0) * (double)n);
        lookup_count_kernel<<<grid, PERM_BLOCK, 0, ctx->stream>>>(LD, d_trace_cols, n, d_tab, (uint32_t)cap, d_mult, d_fl);
        HIP_TRY(ctx, hipGetLastError());
    }
    HelperFlags fl;
    HIP_TRY(ctx, hipMemcpyAsync(&fl, d_fl, sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (fl.exhausted) return smi_fail(ctx, SMI_ERR_BAD_ARG, "lookup_multiplicities: a probe ran through the whole table");
    if (fl.first != ~0ull) {
        const std::string why = "lookup_multiplicities: the tuple of row " + std::to_string(fl.first) + " is in no table row";
        return smi_fail(ctx, SMI_ERR_LOOKUP_MISSING, why.c_str());
    }
    return SMI_OK;
}

int smi_dev_lookup_column(smi_ctx *ctx, const void *lookup_, const uint32_t *d_trace_cols, uint32_t n_cols, uint32_t log_n, const uint64_t *challenges,
                          uint32_t *d_s, size_t s_stride, int *closes) {
    const smi_air_lookup *lk = (const smi_air_lookup *)lookup_;
    if (!ctx || !lk || !d_trace_cols || !challenges || !d_s) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(lookup_args(ctx, lk, n_cols, log_n));
    if (s_stride < (1ull << log_n)) return smi_fail(ctx, SMI_ERR_BAD_ARG, "lookup_column: s_stride < n");
    LookupDev LD;
    lookup_build(ctx->fs.F, ctx->fs.g, lk, challenges, &LD);
    void *tmp = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, lookup_column_tmp_bytes(1ull << log_n), &tmp));
    SMI_TRY(lookup_column_enqueue(ctx, LD, d_trace_cols, log_n, d_s, s_stride, (uint8_t *)tmp));
    LookupFlags fl;
    HIP_TRY(ctx, hipMemcpyAsync(&fl, lookup_column_flags((const uint8_t *)tmp, log_n), sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return lookup_column_verdict(ctx, fl, closes);
}

int smi_dev_air_compose_lookup(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *lookup_, const uint32_t *d_lde, size_t stride,
                               const uint32_t *d_s_lde, size_t s_stride, const uint64_t *challenges, const uint64_t *d_weights, uint32_t *d_out,
                               size_t out_stride) {
    const smi_air_lookup *lk = (const smi_air_lookup *)lookup_;
    if (!ctx || !cfg || !air || !lk || !d_lde || !d_s_lde || !challenges || !d_weights || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    AirHost H;
    SMI_TRY(air_host_tables(ctx, cfg, (const smi_air *)air, &H, nullptr));
    SMI_TRY(lookup_args(ctx, lk, cfg->n_cols, cfg->log_n));
    if (stride < H.dev.N || out_stride < H.dev.N || s_stride < H.dev.N)
        return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_lookup: stride < N, s_stride < N or out_stride < N");
    const size_t b_tab = up16(H.per.table_words * 4), b_vals = up16(H.per.vals.size() * 4);
    void *base = nullptr;   // tables | grouped values | blob
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_vals + H.blob.size() * 4, &base));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, (uint32_t *)((uint8_t *)base + b_tab), (uint32_t *)base));
    SMI_TRY(air_compose_ext_launch(ctx, H, (uint32_t *)((uint8_t *)base + b_tab + b_vals), d_lde, stride, d_weights, d_out, out_stride));
    LookupDev LD;
    lookup_build(ctx->fs.F, ctx->fs.g, lk, challenges, &LD);
    const uint32_t W = cfg->n_cols, K = ((const smi_air *)air)->n_constraints;
    return lookup_compose_enqueue(ctx, LD, H, (uint32_t)cfg->trace_offset, d_lde, stride, d_s_lde, s_stride, d_weights + 4 * (size_t)(W + K), d_out, out_stride);
}

int smi_dev_air_prove_lookup(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const void *lookup_, const uint32_t *d_trace_cols, uint8_t *roots_out,
                             uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits, int *closes) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_lookup *lk = (const smi_air_lookup *)lookup_;
    if (!ctx || !cfg || !air || !lk || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (closes) *closes = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    AirHost H;
    uint64_t E = 0;
    SMI_TRY(air_host_tables(ctx, cfg, air, &H, &E));   // E of the AIR alone; the plan below counts the auxiliary transition of degree 3 in
    SMI_TRY(lookup_args(ctx, lk, cfg->n_cols, cfg->log_n));
    {
        std::string why;
        const int rc = lookup_plan(ctx->fs.F.p, cfg, air, lk, nullptr, &E, &why);
        if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    }
    const size_t n = (size_t)1 << cfg->log_n, N = n << cfg->log_blowup;
    LookupDev LD;
    TwoTreeVariant v;
    v.name = "air_prove_lookup";
    v.A = 1;
    v.tmp_bytes = lookup_column_tmp_bytes(n);
    v.flags_bytes = sizeof(LookupFlags);
    v.columns = [&](const uint64_t *ch, const uint32_t *, uint32_t *d_s, uint8_t *d_tmp) {
        lookup_build(ctx->fs.F, ctx->fs.g, lk, ch, &LD);
        return lookup_column_enqueue(ctx, LD, d_trace_cols, cfg->log_n, d_s, n, d_tmp);
    };
    v.settle = [&](const void *fl) { return lookup_column_verdict(ctx, *(const LookupFlags *)fl, closes); };
    v.compose = [&](const AirHost &Hd, const uint32_t *d_lde, const uint32_t *d_sl, const uint64_t *d_w, uint32_t *d_cw) {
        return lookup_compose_enqueue(ctx, LD, Hd, (uint32_t)cfg->trace_offset, d_lde, N, d_sl, N, d_w, d_cw, N);
    };
    return two_tree_prove(ctx, cfg, H, E, d_trace_cols, v, roots_out, proof, proof_len, top_indices, stage_ms, grind_bits);
}
