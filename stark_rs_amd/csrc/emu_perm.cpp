// emu_perm.cpp -- CPU emulator of the permutation argument's kernels (TEST INFRASTRUCTURE).
//
// emu_perm_column runs the three launches of smi_dev_perm_column in host memory with the kernels' own lane batching and
// block split: perm_lane_column (perm_core.h) for every lane of every workgroup, the workgroup's scan of the lane
// products step by step (perm_scan_step, a loop over the lanes where the kernel has a barrier), the loop of one workgroup
// over the workgroup products PERM_BLOCK at a time, and the propagation.
// emu_air_compose_perm runs emu_air_compose_ext and then air_perm_compose_kernel's grid-stride loop, four points per lane,
// over perm_compose_points.  Same arguments and statuses as the C ABI, with (p, g) in place of a context.
#include <string.h>

#include <string>
#include <vector>

#include "perm_core.h"
#include "tables.h"

extern "C" int emu_air_compose_ext(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const uint32_t *lde, uint64_t stride,
                                   const uint64_t *weights, uint32_t *out, uint64_t out_stride, int force_direct);

namespace {
void load4(const uint32_t *src, uint64_t at, uint64_t len, uint32_t v[4]) {
    for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
}
void store4(uint32_t *dst, uint64_t at, uint64_t len, const uint32_t v[4]) {
    for (int q = 0; q < 4; q++)
        if (at + q < len) dst[at + q] = v[q];
}
// perm_wg_scan of perm.hip: v[tid] -> excl[tid] and the product
Fq wg_scan(const Fq *v, Fq *excl, uint32_t g_m, const Fp &F) {
    static thread_local uint32_t sc[2][4][PERM_BLOCK];
    for (uint32_t tid = 0; tid < PERM_BLOCK; tid++)
        for (int e = 0; e < 4; e++) sc[0][e][tid] = v[tid].c[e];
    int cur = 0;
    for (uint32_t off = 1; off < PERM_BLOCK; off <<= 1) {
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) perm_scan_step(sc[cur], sc[cur ^ 1], tid, off, g_m, F);
        cur ^= 1;
    }
    for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) excl[tid] = tid ? perm_scan_at(sc[cur], tid - 1) : fq_one(F);
    return perm_scan_at(sc[cur], PERM_BLOCK - 1);
}
}  // namespace

extern "C" int emu_perm_column(uint64_t p, uint64_t g, const smi_air_perm *perm, const uint32_t *trace, uint32_t n_cols, uint32_t log_n,
                               const uint64_t *challenges, uint32_t *z, uint64_t z_stride, int *closes, uint64_t *zero_row) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30)) return SMI_ERR_BAD_ARG;
    if (!n_cols || n_cols > 64 || log_n < 1 || log_n > 27) return SMI_ERR_BAD_ARG;
    if (perm_validate(perm, n_cols, nullptr) != SMI_OK) return SMI_ERR_BAD_ARG;
    const Fp F = fs.F;
    const uint64_t n = 1ull << log_n, nb = (n + PERM_TILE - 1) / PERM_TILE;
    if (z_stride < n) return SMI_ERR_BAD_ARG;
    PermDev PD;
    perm_build(F, (uint32_t)g, perm, challenges, &PD);
    std::vector<Fq> bp(nb);
    uint64_t first = ~0ull;
    // perm_block_kernel
    std::vector<Fq> prod(PERM_BLOCK), pre(PERM_BLOCK), zls((size_t)PERM_BLOCK * PERM_ROWS);
    for (uint64_t b = 0; b < nb; b++) {
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
            const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
            uint64_t zr;
            perm_lane_column(
                PD, F, row0, n,
                [&](uint32_t col, uint32_t v[4]) {
                    if (row0 < n) load4(trace + (uint64_t)col * n, row0, n, v);
                    else v[0] = v[1] = v[2] = v[3] = 0u;
                },
                &zls[(size_t)tid * PERM_ROWS], &prod[tid], &zr);
            if (zr < first) first = zr;
        }
        bp[b] = wg_scan(prod.data(), pre.data(), PD.g_m, F);
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
            const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
            if (row0 >= n) break;
            uint32_t o[4][PERM_ROWS];
            for (int q = 0; q < PERM_ROWS; q++) {
                const Fq w = fq_mul(zls[(size_t)tid * PERM_ROWS + q], pre[tid], PD.g_m, F);
                for (int e = 0; e < 4; e++) o[e][q] = w.c[e];
            }
            for (int e = 0; e < 4; e++) store4(z + e * z_stride, row0, n, o[e]);
        }
    }
    // perm_scan_kernel: one workgroup, PERM_BLOCK products at a time
    Fq carry = fq_one(F);
    std::vector<Fq> excl(nb);
    for (uint64_t base = 0; base < nb; base += PERM_BLOCK) {
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) prod[tid] = base + tid < nb ? bp[base + tid] : fq_one(F);
        const Fq tile = wg_scan(prod.data(), pre.data(), PD.g_m, F);
        for (uint32_t tid = 0; tid < PERM_BLOCK && base + tid < nb; tid++) {
            const Fq w = fq_mul(carry, pre[tid], PD.g_m, F);
            for (int e = 0; e < 4; e++) excl[base + tid].c[e] = from_mont(w.c[e], F);
        }
        carry = fq_mul(carry, tile, PD.g_m, F);
    }
    // perm_propagate_kernel
    for (uint64_t b = 0; b < nb; b++) {
        const ExtMul M = ext_mul_prepare(excl[b].c, PD.g_m, F);
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
            const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
            if (row0 >= n) break;
            uint32_t v[4][PERM_ROWS];
            for (int e = 0; e < 4; e++) load4(z + e * z_stride, row0, n, v[e]);
            for (int q = 0; q < PERM_ROWS; q++) {
                const uint32_t a[4] = {v[0][q], v[1][q], v[2][q], v[3][q]};
                uint32_t o[4];
                ext_mul_prepared(a, M, F, o);
                for (int e = 0; e < 4; e++) v[e][q] = o[e];
            }
            for (int e = 0; e < 4; e++) store4(z + e * z_stride, row0, n, v[e]);
        }
    }
    if (zero_row) *zero_row = first;
    if (first != ~0ull) return SMI_ERR_NO_INVERSE;
    if (closes) *closes = from_mont(carry.c[0], F) == 1u && !(carry.c[1] | carry.c[2] | carry.c[3]);
    return SMI_OK;
}

// grid: workgroups of the streaming launch (0: as the library sizes it for 256 compute units)
extern "C" int emu_air_compose_perm(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_perm *perm, const uint32_t *lde,
                                    uint64_t stride, const uint32_t *zl, uint64_t z_stride, const uint64_t *challenges, const uint64_t *weights,
                                    uint32_t *out, uint64_t out_stride, int force_direct, uint32_t grid) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr)) return SMI_ERR_BAD_ARG;
    std::string why;
    const int prc = perm_plan(p, cfg, air, perm, nullptr, nullptr, &why);
    if (prc != SMI_OK) return prc;
    const int rc = emu_air_compose_ext(p, g, cfg, air, lde, stride, weights, out, out_stride, force_direct);
    if (rc != SMI_OK) return rc;
    const uint32_t log_N = cfg->log_n + cfg->log_blowup;
    const Fp F = fs.F;
    AirHost H;
    air_build(F, host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p), cfg, air, &H);
    const AirDev &A = H.dev;
    if (z_stride < A.N) return SMI_ERR_BAD_ARG;
    PermDev PD;
    perm_build(F, (uint32_t)g, perm, challenges, &PD);
    const uint64_t *w = weights + 4 * (uint64_t)(A.W + A.K);
    uint32_t wm[4];
    for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[e], F);
    const ExtMul wb = ext_mul_prepare(wm, PD.g_m, F);
    for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[4 + e], F);
    const ExtMul wt = ext_mul_prepare(wm, PD.g_m, F);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK;
    if (!grid) grid = (uint32_t)(want < 2048 ? want : 2048);
    const uint64_t gstep = (uint64_t)grid * PERM_BLOCK;
    const uint32_t B = 1u << A.log_B, tau_m = air_to_m((uint32_t)cfg->trace_offset, F.p);
    const uint32_t xstep_m = mont_pow(A.omega_m, gstep * PERM_ROWS, F);
    for (uint64_t gid = 0; gid < gstep && gid < groups; gid++) {
        uint32_t x_m = mont_mul(A.h_m, mont_pow(A.omega_m, gid * PERM_ROWS, F), F);
        for (uint64_t gq = gid; gq < groups; gq += gstep) {
            const uint64_t i0 = gq * PERM_ROWS, i1 = (i0 + B) & (A.N - 1);
            uint32_t zc[4][PERM_ROWS], zx[4][PERM_ROWS], acc[4][PERM_ROWS];
            for (int e = 0; e < 4; e++) {
                load4(zl + e * z_stride, i0, A.N, zc[e]);
                load4(zl + e * z_stride, i1, A.N, zx[e]);
                load4(out + e * out_stride, i0, A.N, acc[e]);
            }
            perm_compose_points(
                PD, F, wb, wt, tau_m, A.izt_m, B, i0, x_m, A.omega_m, [&](uint32_t col, uint32_t v[4]) { load4(lde + (uint64_t)col * stride, i0, A.N, v); }, zc,
                zx, acc);
            for (int e = 0; e < 4; e++) store4(out + e * out_stride, i0, A.N, acc[e]);
            x_m = mont_mul(x_m, xstep_m, F);
        }
    }
    return SMI_OK;
}
