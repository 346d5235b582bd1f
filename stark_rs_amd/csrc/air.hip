// air.hip -- AIR constraints over the committed columns: the composition codeword (boundary quotients, transition
// quotients and unconstrained columns under Fiat-Shamir weights), the trace checker and the prover that feeds the
// codeword to Fri::prove.  The definition, the limits and the proof layout are in include/stark_mi.h ("AIR"); the
// per-point evaluator is air_core.h, shared with the CPU emulator (emu_air.cpp).  The verifier is in verify.hip.
//
// air_compose_kernel.  The floor is one read of the W extended columns and one write of the codeword, 4 (W + 1) N
// bytes.  A workgroup walks tiles of T points (grid-stride over the tiles, combine_columns_kernel's shape: the tile
// order does not matter to HBM and a fixed grid keeps the per-workgroup set-up -- the weights, one power -- off the
// per-tile path).  Per tile it stages T + B elements of every column into LDS with 16-byte loads, the halo of B
// wrapping at N, so the next-row operand of point i (index i + B) is read from HBM once, as somebody's this-row
// operand; the evaluator then walks the AIR's terms and fetches operands from LDS (lane j reads address j: no bank
// conflict).  The AIR tables are indexed with wave-uniform values only, so they are scalar loads; x_i is one table
// entry times one per-tile power, then a multiplication per further point; 1 / (x^n - tau^n) is a B-entry table and
// the 1 / Z_c(x_i) share one Fermat inversion per AIR_INV_BATCH values.
//
// Periodic columns are Q more tile rows, staged from tables of L_j = P_j * B values that are read modulo their length
// (air_core.h).  A table is at most a column and usually a few KB, so it comes from L2 and the floor above stands.
// air_periodic_tables builds the tables on the stream with one batched smi_dev_lde per distinct period.
//
// Transition windows (include/stark_mi.h, "AIR: transition windows").  WIN = true instantiates the same kernels for an AIR
// that reads S = 3 or 4 rows: the halo is (S - 1) B points, which air_tile counts against the 64 KB, and an operand's LDS
// address is its row's plus s B.  The two-row instantiations (WIN = false) are the code they were; the launchers pick by
// AirDev::S.  Where no tile fits under the wider halo the direct kernel takes over as before.
#include <string>
#include <vector>

#include "air_core.h"
#include "args_core.h"
#include "deep_core.h"
#include "hash_core.h"
#include "internal.h"
#include "mgpu_core.h"
#include "lookup_core.h"
#include "perm_core.h"
#include "xargs_core.h"
#include "zk_core.h"
#include "zkargs_core.h"

template <int P, bool WIN = false>
__global__ __launch_bounds__(AIR_BLOCK) void air_compose_kernel(AirDev A, Fp F, const uint32_t *__restrict__ cols, size_t stride,
                                                                 const uint64_t *__restrict__ weights, uint32_t T,
                                                                 uint32_t *__restrict__ out) {
    extern __shared__ __align__(16) uint32_t air_lds[];
    uint32_t *w_m = air_lds, *tile = air_lds + AIR_MAX_WEIGHTS;
    const uint32_t threads = blockDim.x, tid = threadIdx.x, pitch = T + (WIN ? (A.S - 1) << A.log_B : 1u << A.log_B);
    for (uint32_t i = tid; i < A.W + A.K; i += threads) w_m[i] = to_mont_u64(weights[i], F);
    const uint32_t step_m = mont_pow(A.omega_m, threads, F);
    const uint64_t tiles = A.N / T;
    // x of the tile's first point: one power per workgroup, then one product per tile (grid-stride: gridDim.x * T further)
    uint32_t xbase_m = mont_mul(A.h_m, mont_pow(A.omega_m, (uint64_t)blockIdx.x * T, F), F);
    const uint32_t xstride_m = mont_pow(A.omega_m, (uint64_t)gridDim.x * T, F);
    for (uint64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const uint64_t base = tl * T;
        __syncthreads();   // the tile of the round before is consumed
        for (uint32_t c = 0; c < A.W; c++)
            for (uint32_t e = tid * 4; e < pitch; e += threads * 4)   // pitch, base and N are multiples of 4: no access straddles the wrap
                *(uint4 *)(tile + c * pitch + e) = *(const uint4 *)(cols + c * stride + ((base + e) & (A.N - 1)));
        for (uint32_t j = 0; j < A.Q; j++) {   // L_j is a multiple of 4 as well: a short table wraps any number of times inside a tile
            const uint32_t *__restrict__ tb = A.ptab + A.pofs[j];
            const uint32_t mask = (1u << A.plog[j]) - 1u;
            for (uint32_t e = tid * 4; e < pitch; e += threads * 4)
                *(uint4 *)(tile + (A.W + j) * pitch + e) = *(const uint4 *)(tb + ((uint32_t)(base + e) & mask));
        }
        __syncthreads();   // tile (and, the first time, the weights) visible
        air_tile_thread<P, WIN>(A, F, w_m, tile, T, threads, base, xbase_m, step_m, tid, out);
        xbase_m = mont_mul(xbase_m, xstride_m, F);   // wave-uniform
    }
}

template <bool WIN = false>
__global__ __launch_bounds__(AIR_BLOCK) void air_direct_kernel(AirDev A, Fp F, const uint32_t *__restrict__ cols, size_t stride,
                                                                const uint64_t *__restrict__ weights, uint32_t *__restrict__ out) {
    __shared__ uint32_t w_m[AIR_MAX_WEIGHTS];
    for (uint32_t i = threadIdx.x; i < A.W + A.K; i += blockDim.x) w_m[i] = to_mont_u64(weights[i], F);
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.N; i += step) air_direct_point<WIN>(A, F, w_m, cols, stride, i, out);
}

// The composition under weights from the quartic extension: air_compose_kernel's tiling, halo and per-tile x, with
// 4 (W + K) weights in LDS (coordinate e of weight j at w_m[e * AIR_MAX_WEIGHTS + j], from weights[4 j + e]) and four output
// columns out_stride apart.  Every quotient is evaluated once per point and added into four accumulators
// (air_core.h air_compose_points_ext); the floor is one read of the columns and four writes, 4 (W + 4) N bytes.
template <int P, bool WIN = false>
__global__ __launch_bounds__(AIR_BLOCK) void air_compose_ext_kernel(AirDev A, Fp F, const uint32_t *__restrict__ cols, size_t stride,
                                                                     const uint64_t *__restrict__ weights, uint32_t T,
                                                                     uint32_t *__restrict__ out, size_t out_stride) {
    extern __shared__ __align__(16) uint32_t air_lds[];
    uint32_t *w_m = air_lds, *tile = air_lds + 4 * AIR_MAX_WEIGHTS;
    const uint32_t threads = blockDim.x, tid = threadIdx.x, pitch = T + (WIN ? (A.S - 1) << A.log_B : 1u << A.log_B);
    for (uint32_t i = tid; i < 4 * (A.W + A.K); i += threads) w_m[(i & 3) * AIR_MAX_WEIGHTS + (i >> 2)] = to_mont_u64(weights[i], F);
    const uint32_t step_m = mont_pow(A.omega_m, threads, F);
    const uint64_t tiles = A.N / T;
    uint32_t xbase_m = mont_mul(A.h_m, mont_pow(A.omega_m, (uint64_t)blockIdx.x * T, F), F);
    const uint32_t xstride_m = mont_pow(A.omega_m, (uint64_t)gridDim.x * T, F);
    for (uint64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const uint64_t base = tl * T;
        __syncthreads();   // the tile of the round before is consumed
        for (uint32_t c = 0; c < A.W; c++)
            for (uint32_t e = tid * 4; e < pitch; e += threads * 4)
                *(uint4 *)(tile + c * pitch + e) = *(const uint4 *)(cols + c * stride + ((base + e) & (A.N - 1)));
        for (uint32_t j = 0; j < A.Q; j++) {
            const uint32_t *__restrict__ tb = A.ptab + A.pofs[j];
            const uint32_t mask = (1u << A.plog[j]) - 1u;
            for (uint32_t e = tid * 4; e < pitch; e += threads * 4)
                *(uint4 *)(tile + (A.W + j) * pitch + e) = *(const uint4 *)(tb + ((uint32_t)(base + e) & mask));
        }
        __syncthreads();   // tile (and, the first time, the weights) visible
        air_tile_thread_ext<P, WIN>(A, F, w_m, tile, T, threads, base, xbase_m, step_m, tid, out, out_stride);
        xbase_m = mont_mul(xbase_m, xstride_m, F);   // wave-uniform
    }
}

template <bool WIN = false>
__global__ __launch_bounds__(AIR_BLOCK) void air_direct_ext_kernel(AirDev A, Fp F, const uint32_t *__restrict__ cols, size_t stride,
                                                                    const uint64_t *__restrict__ weights, uint32_t *__restrict__ out, size_t out_stride) {
    __shared__ uint32_t w_m[4 * AIR_MAX_WEIGHTS];
    for (uint32_t i = threadIdx.x; i < 4 * (A.W + A.K); i += blockDim.x) w_m[(i & 3) * AIR_MAX_WEIGHTS + (i >> 2)] = to_mont_u64(weights[i], F);
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.N; i += step) air_direct_point_ext<WIN>(A, F, w_m, cols, stride, i, out, out_stride);
}

// the trace itself: thread i checks boundary point i (i < nb) and the window of rows i .. i + S - 1 (i <= n - S; S = 2: the
// row pair); the first violation in (kind, index, row) order wins an atomic minimum over the key kind << 63 | index << 32 | row
__global__ __launch_bounds__(256) void air_check_kernel(AirDev A, Fp F, const uint32_t *__restrict__ trace, uint64_t n, uint32_t nb,
                                                         const uint32_t *__restrict__ bnd, unsigned long long *first) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb) {
        const uint32_t col = bnd[3 * i], row = bnd[3 * i + 1], val = bnd[3 * i + 2];
        if (trace[col * n + row] != val) atomicMin(first, ((unsigned long long)i << 32) | row);
    }
    if (i + A.S <= n)
        for (uint32_t k = 0; k < A.K; k++) {
            const uint32_t v = air_constraint(A, F, k, [&](uint32_t var) {   // log_B = 0: periodic operands v_j[(i + s) mod P_j]
                return air_mem_operand_win(A, var, i, [&](uint32_t c, uint32_t s) { return trace[c * n + i + s]; });
            });
            if (v) {
                atomicMin(first, (1ull << 63) | ((unsigned long long)k << 32) | i);
                break;   // a higher k of the same row cannot come first
            }
        }
}

// openings of the W column trees at a, b and -- R == 4 -- (a + B) mod N, (b + B) mod N (mgpu_core.h): one workgroup per
// (test, column)
__global__ __launch_bounds__(64) void air_open_kernel(const MgSide *cols, uint32_t W, const uint64_t *top, uint32_t t, uint32_t R, uint64_t B,
                                                       uint8_t *out) {
    mg_column_open_write_n(cols, W, blockIdx.y, top[blockIdx.x], blockIdx.x, t, 0, out, threadIdx.x, 64, R, B);
}

// openings of the one tree over the rows at the same positions (mgpu_core.h mg_row_open_write): one workgroup per (test,
// position); lanes gather the row's W values from the extended columns and copy the log2 N sibling digests
__global__ __launch_bounds__(64) void air_row_open_kernel(const uint32_t *__restrict__ cols, size_t stride, uint32_t W, const uint8_t *__restrict__ nodes,
                                                           uint32_t depth, const uint64_t *__restrict__ top, uint32_t t, uint32_t R, uint64_t B, uint8_t *out) {
    mg_row_open_write(cols, stride, W, nodes, depth, top[blockIdx.x], blockIdx.x, blockIdx.y, t, out, threadIdx.x, 64, R, B);
}

// the same at the four points of a layer-0 coset of FRI at folding factor 4 (mgpu_core.h mg_row_open4_write), R = 4 or 8
__global__ __launch_bounds__(64) void air_row_open4_kernel(const uint32_t *__restrict__ cols, size_t stride, uint32_t W, const uint8_t *__restrict__ nodes,
                                                            uint32_t depth, const uint64_t *__restrict__ top, uint32_t t, uint32_t R, uint64_t B, uint8_t *out) {
    mg_row_open4_write(cols, stride, W, nodes, depth, top[blockIdx.x], blockIdx.x, blockIdx.y, t, out, threadIdx.x, 64, R, B);
}

// out[q * 2Q + j] = pi_j(x_i), out[q * 2Q + Q + j] = pi_j(w x_i) for i = idx[q]: what the verifier needs of the tables
__global__ __launch_bounds__(64) void air_periodic_gather_kernel(AirDev A, const uint64_t *__restrict__ idx, uint32_t count, uint32_t *__restrict__ out) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    for (uint32_t v = 0; v < 2 * A.Q; v++) out[q * 2 * A.Q + v] = air_periodic_operand(A, v < A.Q ? v : v - A.Q, v >= A.Q ? 1u : 0u, idx[q]);
}

// The periodic tables of H on the stream: the grouped values go to d_vals (H.per.vals.size() words), every group is one
// batched extension into d_tab (H.per.table_words words, 16-byte aligned).  H.per must outlive the copy.
int air_periodic_tables(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, uint32_t *d_vals, uint32_t *d_tab) {
    const AirPeriodic &P = H.per;
    H.dev.ptab = d_tab;
    if (P.groups.empty()) return SMI_OK;
    HIP_TRY(ctx, hipMemcpyAsync(d_vals, P.vals.data(), P.vals.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    for (const AirPeriodGroup &g : P.groups)
        SMI_TRY(smi_dev_lde(ctx, d_vals + g.in_off, g.count, g.log_period, cfg->log_blowup, 1, g.lde_offset, d_tab + g.out_off));
    return SMI_OK;
}

int air_periodic_at(smi_ctx *ctx, const smi_stark_cfg *cfg, AirHost &H, const std::vector<uint64_t> &idx, std::vector<uint32_t> *out) {
    const uint32_t Q = H.dev.Q;
    out->assign(idx.size() * 2 * Q, 0);
    if (!Q || idx.empty()) return SMI_OK;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t b_tab = up16(H.per.table_words * 4), b_vals = up16(H.per.vals.size() * 4), b_blob = up16(H.blob.size() * 4), b_idx = up16(idx.size() * 8);
    void *base = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_vals + b_blob + b_idx + out->size() * 4, &base));
    uint8_t *d = (uint8_t *)base;
    uint32_t *d_tab = (uint32_t *)d, *d_vals = (uint32_t *)(d + b_tab), *d_blob = (uint32_t *)(d + b_tab + b_vals);
    uint64_t *d_idx = (uint64_t *)(d + b_tab + b_vals + b_blob);
    uint32_t *d_out = (uint32_t *)(d + b_tab + b_vals + b_blob + b_idx);
    SMI_TRY(air_periodic_tables(ctx, cfg, H, d_vals, d_tab));
    HIP_TRY(ctx, hipMemcpyAsync(d_blob, H.blob.data(), H.blob.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, idx.data(), idx.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    air_bind(H, d_blob);
    air_periodic_gather_kernel<<<(uint32_t)((idx.size() + 63) / 64), 64, 0, ctx->stream>>>(H.dev, d_idx, (uint32_t)idx.size(), d_out);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out->data(), d_out, out->size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    air_bind(H, H.blob.data());
    H.dev.ptab = nullptr;
    return SMI_OK;
}

namespace {
thread_local std::string g_air_err;

// validated tables of (cfg, air) on the host, bound to host memory
int air_host(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, AirHost *H, uint64_t *E, uint32_t max_window = 2) {
    std::string why;
    const int rc = air_validate(ctx->fs.F.p, cfg, air, nullptr, E, &why, false, false, max_window);
    if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    const uint32_t log_N = cfg->log_n + cfg->log_blowup;
    if (log_N > ctx->fs.K)
        return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    air_build(ctx->fs.F, h_root(ctx, log_N), cfg, air, H);
    return SMI_OK;
}

// the blob to d_blob (room for H.blob.size() words), the launch of the codeword kernel; the periodic tables are in place
// (air_periodic_tables)
int air_launch_compose(smi_ctx *ctx, AirHost &H, uint32_t *d_blob, const uint32_t *d_lde, size_t stride, const uint64_t *d_weights,
                       uint32_t *d_out) {
    HIP_TRY(ctx, hipMemcpyAsync(d_blob, H.blob.data(), H.blob.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    air_bind(H, d_blob);
    const AirDev &A = H.dev;
    const Fp F = ctx->fs.F;
    const uint64_t B = 1ull << A.log_B;
    const bool win = A.S > 2;
    AirTile tl = air_tile(A.W + A.Q, B, A.N, 1, A.S);
    if (B < 4 || (stride & 3) || (((uintptr_t)d_lde) & 15u)) tl.T = 0;   // 16-byte loads need aligned columns
    ProfScope ps(ctx, "air_compose_kernel", 4.0 * (A.W + 1.0) * (double)A.N);
    if (!tl.T) {
        size_t grid = (size_t)((A.N + AIR_BLOCK - 1) / AIR_BLOCK);
        if (grid > 4096) grid = 4096;
        if (win) air_direct_kernel<true><<<(uint32_t)grid, AIR_BLOCK, 0, ctx->stream>>>(A, F, d_lde, stride, d_weights, d_out);
        else air_direct_kernel<<<(uint32_t)grid, AIR_BLOCK, 0, ctx->stream>>>(A, F, d_lde, stride, d_weights, d_out);
    } else {
        const uint64_t tiles = A.N / tl.T;
        const size_t lds = (size_t)AIR_MAX_WEIGHTS * 4 + (size_t)(A.W + A.Q) * (tl.T + (A.S - 1) * B) * 4;
        const uint64_t cap = (uint64_t)ctx->num_cus * 8;
        const uint32_t grid = (uint32_t)(tiles < cap ? tiles : cap);
        if (win) {
            if (tl.P == 4) air_compose_kernel<4, true><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out);
            else if (tl.P == 2) air_compose_kernel<2, true><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out);
            else air_compose_kernel<1, true><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out);
        } else if (tl.P == 4) air_compose_kernel<4><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out);
        else if (tl.P == 2) air_compose_kernel<2><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out);
        else air_compose_kernel<1><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

// air_launch_compose for the extension kernel: four output columns out_stride apart
int air_launch_compose_ext(smi_ctx *ctx, AirHost &H, uint32_t *d_blob, const uint32_t *d_lde, size_t stride, const uint64_t *d_weights,
                           uint32_t *d_out, size_t out_stride) {
    HIP_TRY(ctx, hipMemcpyAsync(d_blob, H.blob.data(), H.blob.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    air_bind(H, d_blob);
    const AirDev &A = H.dev;
    const Fp F = ctx->fs.F;
    const uint64_t B = 1ull << A.log_B;
    const bool win = A.S > 2;
    AirTile tl = air_tile(A.W + A.Q, B, A.N, 4, A.S);
    if (B < 4 || (stride & 3) || (((uintptr_t)d_lde) & 15u)) tl.T = 0;   // 16-byte loads need aligned columns
    ProfScope ps(ctx, "air_compose_ext_kernel", 4.0 * (A.W + 4.0) * (double)A.N);
    if (!tl.T) {
        size_t grid = (size_t)((A.N + AIR_BLOCK - 1) / AIR_BLOCK);
        if (grid > 4096) grid = 4096;
        if (win) air_direct_ext_kernel<true><<<(uint32_t)grid, AIR_BLOCK, 0, ctx->stream>>>(A, F, d_lde, stride, d_weights, d_out, out_stride);
        else air_direct_ext_kernel<<<(uint32_t)grid, AIR_BLOCK, 0, ctx->stream>>>(A, F, d_lde, stride, d_weights, d_out, out_stride);
    } else {
        const uint64_t tiles = A.N / tl.T;
        const size_t lds = (size_t)4 * AIR_MAX_WEIGHTS * 4 + (size_t)(A.W + A.Q) * (tl.T + (A.S - 1) * B) * 4;
        const uint64_t cap = (uint64_t)ctx->num_cus * 8;
        const uint32_t grid = (uint32_t)(tiles < cap ? tiles : cap);
        if (win) {
            if (tl.P == 4) air_compose_ext_kernel<4, true><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out, out_stride);
            else if (tl.P == 2) air_compose_ext_kernel<2, true><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out, out_stride);
            else air_compose_ext_kernel<1, true><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out, out_stride);
        } else if (tl.P == 4) air_compose_ext_kernel<4><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out, out_stride);
        else if (tl.P == 2) air_compose_ext_kernel<2><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out, out_stride);
        else air_compose_ext_kernel<1><<<grid, tl.threads, lds, ctx->stream>>>(A, F, d_lde, stride, d_weights, tl.T, d_out, out_stride);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}
}  // namespace

int smi_air_plan(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint32_t *degree, uint64_t *fri_expansion) {
    g_air_err.clear();
    return air_validate(p, cfg, (const smi_air *)air, degree, fri_expansion, &g_air_err, false, false, SMI_AIR_MAX_WINDOW);
}
const char *smi_air_last_error(void) { return g_air_err.c_str(); }
int smi_air_plan_perm(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *perm, uint32_t *degree, uint64_t *fri_expansion) {
    g_air_err.clear();
    return perm_plan(p, cfg, (const smi_air *)air, (const smi_air_perm *)perm, degree, fri_expansion, &g_air_err);
}
int smi_air_plan_lookup(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *lookup, uint32_t *degree, uint64_t *fri_expansion) {
    g_air_err.clear();
    return lookup_plan(p, cfg, (const smi_air *)air, (const smi_air_lookup *)lookup, degree, fri_expansion, &g_air_err);
}
int smi_air_plan_args(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *args, uint32_t *degree, uint64_t *fri_expansion) {
    g_air_err.clear();
    return args_plan(p, cfg, (const smi_air *)air, (const smi_air_args *)args, degree, fri_expansion, &g_air_err);
}
int smi_air_plan_xargs(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint32_t *degree, uint64_t *fri_expansion) {
    g_air_err.clear();
    return xargs_plan(p, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, degree, fri_expansion, &g_air_err);
}
// out-of-domain sampling (deep_core.h): the plan, and the proof length of a planned shape
int smi_air_plan_deep(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint32_t *degree, uint32_t *segments) {
    g_air_err.clear();
    return deep_plan(p, cfg, (const smi_air *)air, degree, segments, &g_air_err, SMI_AIR_MAX_WINDOW);
}
int smi_air_deep_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, size_t *proof_len) {
    g_air_err.clear();
    uint32_t D = 0;
    const int rc = deep_plan(p, cfg, (const smi_air *)air, nullptr, &D, &g_air_err, SMI_AIR_MAX_WINDOW);
    if (rc == SMI_OK && proof_len) *proof_len = deep_proof_len(cfg, D, air_window((const smi_air *)air));
    return rc;
}
// ... with an argument list (xargs_core.h)
int smi_air_plan_deep_xargs(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint32_t *degree, uint32_t *segments) {
    g_air_err.clear();
    return deep_xargs_plan(p, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, degree, segments, &g_air_err);
}
int smi_air_deep_xargs_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, size_t *proof_len) {
    g_air_err.clear();
    uint32_t D = 0;
    const int rc = deep_xargs_plan(p, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, nullptr, &D, &g_air_err);
    if (rc == SMI_OK && proof_len) *proof_len = deep_args_proof_len(cfg, ((const smi_air_xargs *)xargs)->count, D);
    return rc;
}
// ... over coset leaves (deep_core.h): the plans above, the number of folds of FRI at folding factor 4 and the proof length
int smi_air_deep_fold4_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint64_t *folds, size_t *proof_len) {
    g_air_err.clear();
    uint32_t D = 0;
    const int rc = deep_plan(p, cfg, (const smi_air *)air, nullptr, &D, &g_air_err, SMI_AIR_MAX_WINDOW);
    if (rc != SMI_OK) return rc;
    const size_t len = deep_fold4_proof_len(cfg, 0, D, folds, air_window((const smi_air *)air));
    if (proof_len) *proof_len = len;
    return SMI_OK;
}
int smi_air_deep_xargs_fold4_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint64_t *folds, size_t *proof_len) {
    g_air_err.clear();
    uint32_t D = 0;
    const int rc = deep_xargs_plan(p, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, nullptr, &D, &g_air_err);
    if (rc != SMI_OK) return rc;
    const size_t len = deep_fold4_proof_len(cfg, ((const smi_air_xargs *)xargs)->count, D, folds);
    if (proof_len) *proof_len = len;
    return SMI_OK;
}
// zero-knowledge DEEP proofs (zk_core.h): the plan over the derived AIR
int smi_air_plan_deep_zk(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint32_t *degree, uint32_t *segments, uint32_t *k_t, uint32_t *k_s) {
    g_air_err.clear();
    return zk_plan(p, cfg, (const smi_air *)air, degree, segments, k_t, k_s, &g_air_err);
}
int smi_air_deep_zk_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, uint64_t *folds, size_t *proof_len) {
    g_air_err.clear();
    uint32_t Dp = 0;
    const int rc = zk_plan(p, cfg, (const smi_air *)air, nullptr, &Dp, nullptr, nullptr, &g_air_err);
    if (rc != SMI_OK) return rc;
    const size_t len = zk_proof_len(cfg, Dp, folds);
    if (proof_len) *proof_len = len;
    return SMI_OK;
}
// ... with an argument list (zkargs_core.h)
int smi_air_plan_deep_zk_xargs(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint32_t *degree, uint32_t *segments, uint32_t *k_t,
                               uint32_t *k_s) {
    g_air_err.clear();
    return zkx_plan(p, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, degree, segments, k_t, k_s, &g_air_err);
}
int smi_air_deep_zk_xargs_layout(uint64_t p, const smi_stark_cfg *cfg, const void *air, const void *xargs, uint64_t *folds, size_t *proof_len) {
    g_air_err.clear();
    uint32_t Dp = 0;
    const int rc = zkx_plan(p, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, nullptr, &Dp, nullptr, nullptr, &g_air_err);
    if (rc != SMI_OK) return rc;
    const size_t len = zkx_proof_len(cfg, ((const smi_air_xargs *)xargs)->count, Dp, folds);
    if (proof_len) *proof_len = len;
    return SMI_OK;
}
// what perm.hip and lookup.hip share with the provers of this file (internal.h)
int air_host_tables(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, AirHost *H, uint64_t *E) { return air_host(ctx, cfg, air, H, E); }
int air_compose_ext_launch(smi_ctx *ctx, AirHost &H, uint32_t *d_blob, const uint32_t *d_lde, size_t stride, const uint64_t *d_weights, uint32_t *d_out,
                           size_t out_stride) {
    return air_launch_compose_ext(ctx, H, d_blob, d_lde, stride, d_weights, d_out, out_stride);
}
int launch_air_row_open(smi_ctx *ctx, const uint32_t *d_cols, size_t stride, uint32_t W, const uint8_t *d_nodes, uint32_t depth, const uint64_t *d_top,
                        uint32_t t, uint32_t R, uint64_t B, uint8_t *d_out) {
    air_row_open_kernel<<<dim3(t, R), 64, 0, ctx->stream>>>(d_cols, stride, W, d_nodes, depth, d_top, t, R, B, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return SMI_OK;
}

int smi_dev_air_compose(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_lde, size_t stride,
                        const uint64_t *d_weights, uint32_t *d_out) {
    if (!ctx || !cfg || !air || !d_lde || !d_weights || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    AirHost H;
    SMI_TRY(air_host(ctx, cfg, (const smi_air *)air, &H, nullptr, SMI_AIR_MAX_WINDOW));
    if (stride < H.dev.N) return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose: stride < N");
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t b_tab = up16(H.per.table_words * 4), b_vals = up16(H.per.vals.size() * 4);
    void *base = nullptr;   // tables | grouped values | blob
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_vals + H.blob.size() * 4, &base));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, (uint32_t *)((uint8_t *)base + b_tab), (uint32_t *)base));
    return air_launch_compose(ctx, H, (uint32_t *)((uint8_t *)base + b_tab + b_vals), d_lde, stride, d_weights, d_out);
}

int smi_dev_air_compose_ext(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_lde, size_t stride,
                            const uint64_t *d_weights, uint32_t *d_out, size_t out_stride) {
    if (!ctx || !cfg || !air || !d_lde || !d_weights || !d_out) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(ext_field_check(ctx));
    AirHost H;
    SMI_TRY(air_host(ctx, cfg, (const smi_air *)air, &H, nullptr, SMI_AIR_MAX_WINDOW));
    if (stride < H.dev.N || out_stride < H.dev.N) return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_compose_ext: stride < N or out_stride < N");
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t b_tab = up16(H.per.table_words * 4), b_vals = up16(H.per.vals.size() * 4);
    void *base = nullptr;   // tables | grouped values | blob
    SMI_TRY(ctx_tmp(ctx, 3, b_tab + b_vals + H.blob.size() * 4, &base));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, (uint32_t *)((uint8_t *)base + b_tab), (uint32_t *)base));
    return air_launch_compose_ext(ctx, H, (uint32_t *)((uint8_t *)base + b_tab + b_vals), d_lde, stride, d_weights, d_out, out_stride);
}

int smi_dev_air_check(smi_ctx *ctx, const void *air_, uint32_t n_cols, uint32_t log_n, const uint32_t *d_trace_cols, int *ok,
                      uint32_t *constraint, uint64_t *row) {
    const smi_air *air = (const smi_air *)air_;
    if (!ctx || !air || !d_trace_cols || !ok) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *ok = 0;
    smi_stark_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_cols = n_cols;
    cfg.log_n = log_n;
    std::string why;
    const int rc = air_validate(ctx->fs.F.p, &cfg, air, nullptr, nullptr, &why, true, false, SMI_AIR_MAX_WINDOW);
    if (rc != SMI_OK) return smi_fail(ctx, rc, why.c_str());
    AirHost H;
    air_build(ctx->fs.F, 1, &cfg, air, &H, true);
    const uint32_t nb = air->n_boundary;
    const size_t words = H.blob.size(), n_per = H.per.vals.size(), total = words + 3 * (size_t)nb + n_per + 2;
    std::vector<uint32_t> up(H.blob);   // blob | boundary triples | periodic values (the tables of the trace itself)
    up.reserve(total);
    for (uint32_t j = 0; j < nb; j++) {
        up.push_back(air->boundary_col[j]);
        up.push_back((uint32_t)air->boundary_row[j]);
        up.push_back((uint32_t)air->boundary_value[j]);
    }
    up.insert(up.end(), H.per.vals.begin(), H.per.vals.end());
    void *d_blob = nullptr;
    SMI_TRY(ctx_tmp(ctx, 3, total * 4 + 16, &d_blob));
    unsigned long long *d_first = (unsigned long long *)((uint8_t *)d_blob + ((total * 4 + 7) & ~(size_t)7));
    HIP_TRY(ctx, hipMemcpyAsync(d_blob, up.data(), up.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_first, 0xff, 8, ctx->stream));
    air_bind(H, (const uint32_t *)d_blob);
    H.dev.ptab = (const uint32_t *)d_blob + words + 3 * (size_t)nb;
    const uint64_t n = 1ull << log_n, work = n > nb ? n : nb;
    air_check_kernel<<<(uint32_t)((work + 255) / 256), 256, 0, ctx->stream>>>(H.dev, ctx->fs.F, d_trace_cols, n, nb, (const uint32_t *)d_blob + words,
                                                                             d_first);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long first = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&first, d_first, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (first == ~0ull) {
        *ok = 1;
        return SMI_OK;
    }
    const bool transition = first >> 63;
    const uint32_t idx = (uint32_t)((first >> 32) & 0x7fffffffu);
    const uint64_t r = first & 0xffffffffull;
    if (constraint) *constraint = transition ? nb + idx : idx;
    if (row) *row = r;
    const uint32_t S = air_window(air);
    ctx->err = transition ? "air_check: transition constraint " + std::to_string(idx) + " is violated on rows " + std::to_string(r) + (S > 2 ? " .. " : " and ") + std::to_string(r + S - 1)
                          : "air_check: boundary point " + std::to_string(idx) + " (column " + std::to_string(air->boundary_col[idx]) + ", row " + std::to_string(r) +
                                ") does not hold value " + std::to_string(air->boundary_value[idx]);
    return SMI_OK;
}

// The prover of both commitments.  rows == false: one tree per column, the transcript of the W roots and the K constraint
// indices, W paths per opened position (smi_dev_air_prove).  rows == true: one tree over the rows, the transcript of its
// root and the W + K indices, one path per opened position (smi_dev_air_prove_rows).  Everything else -- the extension, the
// periodic tables, the composition, FRI, the copy-back -- is the same code.
// ext (with rows): the weights are elements of the quartic extension -- four counters and four challenges per weight --, the
// composition codeword is four coordinate columns and FRI runs over F_q (smi_dev_air_prove_ext).
// grind (with ext): the proof-of-work difficulty of the FRI part, or SMI_GRIND_NONE (smi_dev_air_prove_ext_pow).
// fold4 (with ext and a difficulty): FRI at folding factor 4 and the rows at the four points of every layer-0 coset
// (smi_dev_air_prove_ext_fold4); every other caller passes false and runs what it ran before.
static int air_prove_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, const uint32_t *d_trace_cols, uint8_t *column_roots,
                          uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, bool rows, bool ext = false,
                          int grind = SMI_GRIND_NONE, bool fold4 = false) {
    AirHost H;
    uint64_t E = 0;
    SMI_TRY(air_host(ctx, cfg, air, &H, &E));
    if (fold4) {   // without a fold there is no layer-0 coset record to compare the composition with
        const smi_fri_cfg fc0 = trace_fri_cfg(ctx, cfg, E);
        const FriFold4Layout lay = fri_layout_fold4(fc0);
        if (lay.R2 && lay.F == 0) return smi_fail(ctx, SMI_ERR_BAD_ARG, AIR_FOLD4_NO_LAYER);
    }
    const uint32_t W = cfg->n_cols, K = air->n_constraints, log_N = cfg->log_n + cfg->log_blowup;
    const size_t N = (size_t)1 << log_N;
    SMI_TRY(arena_reset(ctx));
    StageTimer tm(ctx, 5, stage_ms != nullptr);
    HIP_TRY(ctx, tm.create());

    const size_t tree_stride = 2 * N * 32;
    const uint32_t n_trees = rows ? 1u : W;
    uint32_t *d_lde = (uint32_t *)arena_alloc(ctx, (size_t)W * N * 4);
    const uint32_t NE = ext ? 4 : 1;   // coordinates per weight and per codeword element
    uint32_t *d_cw = (uint32_t *)arena_alloc(ctx, (size_t)NE * N * 4);
    uint64_t *d_weights = (uint64_t *)arena_alloc(ctx, 8 * (size_t)NE * (W + K));
    uint32_t *d_blob = (uint32_t *)arena_alloc(ctx, H.blob.size() * 4);
    uint8_t *tree_base = (uint8_t *)arena_alloc(ctx, tree_stride * n_trees);
    uint32_t *d_ptab = nullptr, *d_pvals = nullptr;
    if (H.dev.Q) {
        d_ptab = (uint32_t *)arena_alloc(ctx, H.per.table_words * 4);
        d_pvals = (uint32_t *)arena_alloc(ctx, H.per.vals.size() * 4);
    }
    if (!d_lde || !d_cw || !d_weights || !d_blob || !tree_base || (H.dev.Q && (!d_ptab || !d_pvals)))
        return smi_fail(ctx, SMI_ERR_OOM, "air_prove: device memory");
    tm.mark();
    SMI_TRY(smi_dev_lde(ctx, d_trace_cols, W, cfg->log_n, cfg->log_blowup, cfg->trace_offset, cfg->lde_offset, d_lde));
    tm.mark();
    if (rows) SMI_TRY(launch_merkle_rows(ctx, d_lde, W, N, N, tree_base));
    else SMI_TRY(launch_merkle_batch(ctx, d_lde, N, tree_base, W, N, tree_stride));
    tm.mark();
    // The roots make one small round trip: the transcript (roots, then the indices) and its weights
    // are computed on the host, where fri_run's seed is computed anyway (transcript_core.h).
    std::vector<uint8_t> roots(32 * (size_t)n_trees);
    HIP_TRY(ctx, hipMemcpy2DAsync(roots.data(), 32, tree_base + (2 * N - 2) * 32, tree_stride, 32, n_trees, hipMemcpyDeviceToHost, ctx->stream));
    SMI_TRY(air_periodic_tables(ctx, cfg, H, d_pvals, d_ptab));   // part of the compose stage, queued before the host waits for the roots
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    Transcript tr;
    std::vector<uint64_t> weights;   // NE (W + K) of them
    if (ext) transcript_ext(tr, roots.data(), W, K, &weights);
    else if (rows) transcript_rows(tr, roots.data(), W, K, &weights);
    else transcript_columns(tr, roots.data(), W, K, &weights);
    const FsSeed seed = tr.seed();
    if (column_roots) memcpy(column_roots, roots.data(), roots.size());
    HIP_TRY(ctx, hipMemcpyAsync(d_weights, weights.data(), 8 * weights.size(), hipMemcpyHostToDevice, ctx->stream));
    if (ext) SMI_TRY(air_launch_compose_ext(ctx, H, d_blob, d_lde, N, d_weights, d_cw, N));
    else SMI_TRY(air_launch_compose(ctx, H, d_blob, d_lde, N, d_weights, d_cw));
    tm.mark();
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, E);
    FriResult res;
    FriExtResult xres;
    if (ext) {
        if (fold4) SMI_TRY(fri_run_ext_fold4(ctx, &fc, &seed, d_cw, N, N, false, &xres, (uint32_t)grind));
        else SMI_TRY(fri_run_ext(ctx, &fc, &seed, d_cw, N, N, false, &xres, grind));
    } else {
        FriRequest rq(&fc, d_cw, N, true);
        rq.reset_arena = false;
        rq.seed = &seed;
        SMI_TRY(fri_run(ctx, rq, &res));
    }
    std::vector<uint8_t> &bytes = ext ? xres.proof : res.proof;
    std::vector<uint64_t> &top = ext ? xres.top : res.top;
    if (top_indices) memcpy(top_indices, top.data(), 8 * (size_t)cfg->num_colinearity_tests);
    else top_indices = top.data();   // the column openings need the top-level indices either way
    tm.mark();
    if (cfg->num_colinearity_tests && rows) {
        const uint32_t t = (uint32_t)cfg->num_colinearity_tests, R = (K ? 4u : 2u) * (fold4 ? 2u : 1u);
        const size_t ob = (size_t)mg_row_open_bytes(W, t, log_N, R);
        uint64_t *d_top = (uint64_t *)arena_alloc(ctx, 8 * (size_t)t);
        uint8_t *d_open = (uint8_t *)arena_alloc(ctx, ob);
        if (!d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, "air_prove: row openings");
        HIP_TRY(ctx, hipMemcpyAsync(d_top, top_indices, 8 * (size_t)t, hipMemcpyHostToDevice, ctx->stream));
        if (fold4) air_row_open4_kernel<<<dim3(t, R), 64, 0, ctx->stream>>>(d_lde, N, W, tree_base, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open);
        else air_row_open_kernel<<<dim3(t, R), 64, 0, ctx->stream>>>(d_lde, N, W, tree_base, log_N, d_top, t, R, 1ull << cfg->log_blowup, d_open);
        HIP_TRY(ctx, hipGetLastError());
        const size_t at = bytes.size();
        bytes.resize(at + ob);
        HIP_TRY(ctx, hipMemcpyAsync(bytes.data() + at, d_open, ob, hipMemcpyDeviceToHost, ctx->stream));
    } else if (cfg->num_colinearity_tests) {
        const uint32_t t = (uint32_t)cfg->num_colinearity_tests, R = K ? 4u : 2u;
        std::vector<MgSide> sides(W);
        for (uint32_t c = 0; c < W; c++) {
            MgSide &sd = sides[c];
            sd.cw = d_lde + (size_t)c * N; sd.nodes = tree_base + c * tree_stride; sd.top = nullptr; sd.len = N; sd.blk = N; sd.depth_local = log_N; sd.depth_top = 0;
        }
        const size_t ob = (size_t)mg_column_open_bytes(W, t, log_N, R);
        MgSide *d_sides = (MgSide *)arena_alloc(ctx, sizeof(MgSide) * W);
        uint64_t *d_top = (uint64_t *)arena_alloc(ctx, 8 * (size_t)t);
        uint8_t *d_open = (uint8_t *)arena_alloc(ctx, ob);
        if (!d_sides || !d_top || !d_open) return smi_fail(ctx, SMI_ERR_OOM, "air_prove: column openings");
        HIP_TRY(ctx, hipMemcpyAsync(d_sides, sides.data(), sizeof(MgSide) * W, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_top, top_indices, 8 * (size_t)t, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_open, 0, ob, ctx->stream));
        air_open_kernel<<<dim3(t, W), 64, 0, ctx->stream>>>(d_sides, W, d_top, t, R, 1ull << cfg->log_blowup, d_open);
        HIP_TRY(ctx, hipGetLastError());
        const size_t at = bytes.size();
        bytes.resize(at + ob);
        HIP_TRY(ctx, hipMemcpyAsync(bytes.data() + at, d_open, ob, hipMemcpyDeviceToHost, ctx->stream));
    }
    tm.mark();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    tm.write(stage_ms);
    return smi_proof_out(ctx, bytes, proof, proof_len);
}

int smi_dev_air_prove(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t *column_roots,
                      uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms) {
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (cfg->row_leaves) return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_prove: column trees only (row_leaves must be 0; smi_dev_air_prove_rows commits to one tree over the rows)");
    return air_prove_impl(ctx, cfg, (const smi_air *)air, d_trace_cols, column_roots, proof, proof_len, top_indices, stage_ms, false);
}

int smi_dev_air_prove_rows(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t row_root[32],
                           uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms) {
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    return air_prove_impl(ctx, cfg, (const smi_air *)air, d_trace_cols, row_root, proof, proof_len, top_indices, stage_ms, true);
}

int smi_dev_air_prove_ext(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t row_root[32],
                          uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms) {
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(ext_field_check(ctx));
    return air_prove_impl(ctx, cfg, (const smi_air *)air, d_trace_cols, row_root, proof, proof_len, top_indices, stage_ms, true, true);
}

int smi_dev_air_prove_ext_pow(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t row_root[32],
                              uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return air_prove_impl(ctx, cfg, (const smi_air *)air, d_trace_cols, row_root, proof, proof_len, top_indices, stage_ms, true, true, (int)grind_bits);
}

// smi_dev_air_prove_ext_pow over FRI at folding factor 4 (include/stark_mi.h, "Extension FRI, folding factor 4")
int smi_dev_air_prove_ext_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint32_t *d_trace_cols, uint8_t row_root[32],
                                uint8_t **proof, size_t *proof_len, uint64_t *top_indices, double *stage_ms, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !d_trace_cols || !proof || !proof_len) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return air_prove_impl(ctx, cfg, (const smi_air *)air, d_trace_cols, row_root, proof, proof_len, top_indices, stage_ms, true, true, (int)grind_bits, true);
}
