// emu_deep.cpp -- CPU emulator of the out-of-domain sampling kernels (TEST INFRASTRUCTURE).
//
// emu_poly_eval_ext runs the two launches of smi_dev_poly_eval_ext in host memory with the kernels' own block split and
// lane bodies (deep_core.h): deep_eval_lane for every lane of every workgroup, the workgroup's sum as a loop over the lanes
// where the kernel shuffles, then deep_eval_combine_lane for every lane of the one workgroup per (column, point).
// emu_deep_compose runs deep_compose_kernel's grid-stride loop, four points per lane, over deep_compose_points.
// emu_deep_ood_sides, emu_deep_constraint and emu_deep_q_at expose the verifier's host arithmetic.  Same arguments and
// statuses as the C ABI, with (p, g) in place of a context.
#include <string.h>

#include <string>
#include <vector>

#include "deep_core.h"
#include "tables.h"

namespace {
void load4(const uint32_t *src, uint64_t at, uint64_t len, uint32_t v[4]) {
    for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
}
void store4(uint32_t *dst, uint64_t at, uint64_t len, const uint32_t v[4]) {
    for (int q = 0; q < 4; q++)
        if (at + q < len) dst[at + q] = v[q];
}
bool setup(uint64_t p, uint64_t g, FieldSetup *fs, int *rc) {
    if (!field_setup(p, g, fs)) return *rc = SMI_ERR_UNSUPPORTED_PRIME, false;
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30)) return *rc = SMI_ERR_BAD_ARG, false;
    return true;
}
bool point(const uint64_t *v, uint64_t p, FqH *z) {
    for (int e = 0; e < 4; e++) {
        if (v[e] >= p) return false;
        z->c[e] = (uint32_t)v[e];
    }
    return true;
}
}  // namespace

extern "C" int emu_poly_eval_ext(uint64_t p, uint64_t g, const uint32_t *coeffs, uint32_t n_cols, uint64_t n_coeffs, uint64_t stride, const uint64_t *points,
                                 uint32_t n_points, uint64_t *out) {
    FieldSetup fs;
    int rc = SMI_OK;
    if (!setup(p, g, &fs, &rc)) return rc;
    if (!n_cols || !n_coeffs || stride < n_coeffs || n_points < 1 || n_points > DEEP_MAX_POINTS) return SMI_ERR_BAD_ARG;
    const Fp F = fs.F;
    const uint32_t P = n_points, g_m = air_to_m((uint32_t)g, F.p);
    FqH z[DEEP_MAX_POINTS];
    for (uint32_t k = 0; k < P; k++)
        if (!point(points + 4 * k, p, &z[k])) return SMI_ERR_NON_CANONICAL;
    std::vector<uint32_t> tab;
    deep_eval_build(F, (uint32_t)g, P, z, &tab);
    const uint64_t nb = deep_eval_blocks(n_coeffs);
    std::vector<uint32_t> part((size_t)n_cols * nb * P * 4, 0);
    // deep_eval_kernel
    for (uint64_t b = 0; b < nb; b++)
        for (uint32_t c = 0; c < n_cols; c++) {
            uint32_t sum[DEEP_MAX_POINTS][4] = {};
            for (uint32_t tid = 0; tid < DEEP_BLOCK; tid++) {
                uint32_t a[DEEP_ROWS];
                load4(coeffs + (size_t)c * stride, b * DEEP_TILE + DEEP_ROWS * tid, n_coeffs, a);
                for (uint32_t k = 0; k < P; k++) {
                    uint32_t tw[4][DEEP_ROWS], acc[4];
                    for (int e = 0; e < 4; e++)
                        for (int q = 0; q < DEEP_ROWS; q++) tw[e][q] = tab[(size_t)(k * 4 + e) * DEEP_TILE + DEEP_ROWS * tid + q];
                    deep_eval_lane(a, tw, F, acc);
                    for (int e = 0; e < 4; e++) sum[k][e] = fp_add(sum[k][e], acc[e], F.p);
                }
            }
            for (uint32_t k = 0; k < P; k++)
                for (int e = 0; e < 4; e++) part[(((size_t)c * nb + b) * P + k) * 4 + e] = sum[k][e];
        }
    // deep_eval_combine_kernel
    for (uint32_t c = 0; c < n_cols; c++)
        for (uint32_t k = 0; k < P; k++) {
            uint32_t sum[4] = {0, 0, 0, 0};
            for (uint32_t tid = 0; tid < DEEP_BLOCK; tid++) {
                uint32_t acc[4];
                deep_eval_combine_lane(&part[((size_t)c * nb * P + k) * 4], P * 4, (uint32_t)nb, tid, &tab[deep_eval_tp_at(P) + (size_t)(k * DEEP_BLOCK + tid) * 4],
                                       &tab[deep_eval_st_at(P) + 4 * k], g_m, F, acc);
                for (int e = 0; e < 4; e++) sum[e] = fp_add(sum[e], acc[e], F.p);
            }
            for (int e = 0; e < 4; e++) out[((size_t)c * P + k) * 4 + e] = sum[e];
        }
    return SMI_OK;
}

// smi_dev_poly_eval_ext_shifts: the same two launches over a table per point z w^s
extern "C" int emu_poly_eval_ext_shifts(uint64_t p, uint64_t g, const uint32_t *coeffs, uint32_t n_cols, uint64_t n_coeffs, uint64_t stride, const uint64_t *z,
                                        uint64_t w, uint32_t n_shifts, uint64_t *out) {
    FieldSetup fs;
    int rc = SMI_OK;
    if (!setup(p, g, &fs, &rc)) return rc;
    if (!n_cols || !n_coeffs || stride < n_coeffs || n_shifts < 1 || n_shifts > DEEP_MAX_SHIFTS) return SMI_ERR_BAD_ARG;
    if (w >= p) return SMI_ERR_NON_CANONICAL;
    const Fp F = fs.F;
    const uint32_t P = n_shifts, g_m = air_to_m((uint32_t)g, F.p);
    FqH pts[DEEP_MAX_SHIFTS];
    if (!point(z, p, &pts[0])) return SMI_ERR_NON_CANONICAL;
    for (uint32_t k = 1; k < P; k++) pts[k] = fqh_scale(pts[k - 1], (uint32_t)w, F.p);
    std::vector<uint32_t> tab;
    deep_eval_build(F, (uint32_t)g, P, pts, &tab);
    const uint64_t nb = deep_eval_blocks(n_coeffs);
    std::vector<uint32_t> part((size_t)n_cols * nb * P * 4, 0);
    for (uint64_t b = 0; b < nb; b++)
        for (uint32_t c = 0; c < n_cols; c++) {
            uint32_t sum[DEEP_MAX_SHIFTS][4] = {};
            for (uint32_t tid = 0; tid < DEEP_BLOCK; tid++) {
                uint32_t a[DEEP_ROWS];
                load4(coeffs + (size_t)c * stride, b * DEEP_TILE + DEEP_ROWS * tid, n_coeffs, a);
                for (uint32_t k = 0; k < P; k++) {
                    uint32_t tw[4][DEEP_ROWS], acc[4];
                    for (int e = 0; e < 4; e++)
                        for (int q = 0; q < DEEP_ROWS; q++) tw[e][q] = tab[(size_t)(k * 4 + e) * DEEP_TILE + DEEP_ROWS * tid + q];
                    deep_eval_lane(a, tw, F, acc);
                    for (int e = 0; e < 4; e++) sum[k][e] = fp_add(sum[k][e], acc[e], F.p);
                }
            }
            for (uint32_t k = 0; k < P; k++)
                for (int e = 0; e < 4; e++) part[(((size_t)c * nb + b) * P + k) * 4 + e] = sum[k][e];
        }
    for (uint32_t c = 0; c < n_cols; c++)
        for (uint32_t k = 0; k < P; k++) {
            uint32_t sum[4] = {0, 0, 0, 0};
            for (uint32_t tid = 0; tid < DEEP_BLOCK; tid++) {
                uint32_t acc[4];
                deep_eval_combine_lane(&part[((size_t)c * nb * P + k) * 4], P * 4, (uint32_t)nb, tid, &tab[deep_eval_tp_at(P) + (size_t)(k * DEEP_BLOCK + tid) * 4],
                                       &tab[deep_eval_st_at(P) + 4 * k], g_m, F, acc);
                for (int e = 0; e < 4; e++) sum[e] = fp_add(sum[e], acc[e], F.p);
            }
            for (int e = 0; e < 4; e++) out[((size_t)c * P + k) * 4 + e] = sum[e];
        }
    return SMI_OK;
}

namespace {
template <int S>
void emu_window_lanes(const uint32_t *tab, uint32_t W, uint32_t D, uint32_t g_m, const Fp &F, uint32_t h_m, uint32_t omega_m, uint64_t N, uint32_t grid,
                      const uint32_t *lde, uint64_t stride, const uint32_t *seg, uint64_t seg_stride, uint32_t *out, uint64_t out_stride) {
    const uint64_t groups = N / DEEP_ROWS, gstep = (uint64_t)grid * DEEP_BLOCK;
    const uint32_t xstep_m = mont_pow(omega_m, gstep * DEEP_ROWS, F);
    for (uint64_t gid = 0; gid < gstep && gid < groups; gid++) {
        uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * DEEP_ROWS, F), F);
        for (uint64_t gq = gid; gq < groups; gq += gstep) {
            const uint64_t i0 = gq * DEEP_ROWS;
            uint32_t o[4][DEEP_ROWS];
            deep_compose_window_points<S>(
                tab, W, D, g_m, F, x_m, omega_m, [&](uint32_t c, uint32_t v[4]) { load4(lde + (uint64_t)c * stride, i0, N, v); },
                [&](uint32_t col, uint32_t v[4]) { load4(seg + (uint64_t)col * seg_stride, i0, N, v); }, o);
            for (int e = 0; e < 4; e++) store4(out + e * out_stride, i0, N, o[e]);
            x_m = mont_mul(x_m, xstep_m, F);
        }
    }
}
}  // namespace

// smi_dev_deep_compose_window: deep_compose_window_kernel's grid-stride loop (window = 2: emu_deep_compose)
extern "C" int emu_deep_compose(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, uint32_t n_segments, const uint32_t *lde, uint64_t stride, const uint32_t *seg,
                                uint64_t seg_stride, const uint64_t *z, const uint64_t *ood, const uint64_t *challenges, uint32_t *out, uint64_t out_stride,
                                uint32_t grid);
extern "C" int emu_deep_compose_window(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, uint32_t window, uint32_t n_segments, const uint32_t *lde, uint64_t stride,
                                       const uint32_t *seg, uint64_t seg_stride, const uint64_t *z, const uint64_t *ood, const uint64_t *challenges, uint32_t *out,
                                       uint64_t out_stride, uint32_t grid) {
    if (window == 2) return emu_deep_compose(p, g, cfg, n_segments, lde, stride, seg, seg_stride, z, ood, challenges, out, out_stride, grid);
    if (window < 2 || window > SMI_AIR_MAX_WINDOW) return SMI_ERR_BAD_ARG;
    FieldSetup fs;
    int rc = SMI_OK;
    if (!setup(p, g, &fs, &rc)) return rc;
    const Fp F = fs.F;
    const uint32_t W = cfg->n_cols, D = n_segments, S = window, log_N = cfg->log_n + cfg->log_blowup;
    if (!W || W > 64 || !D || D > DEEP_MAX_SEGMENTS || cfg->log_n < 1 || cfg->log_blowup < 2 || log_N > 27 || log_N > fs.K) return SMI_ERR_BAD_ARG;
    const uint64_t N = 1ull << log_N;
    if (stride < N || seg_stride < N || out_stride < N || !cfg->lde_offset || cfg->lde_offset >= p) return SMI_ERR_BAD_ARG;
    FqH zq;
    if (!point(z, p, &zq)) return SMI_ERR_NON_CANONICAL;
    if (fqh_in_base(zq)) return SMI_ERR_BAD_ARG;
    for (size_t i = 0; i < 4 * ((size_t)S * W + D); i++)
        if (ood[i] >= p) return SMI_ERR_NON_CANONICAL;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), F.p), omega = host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p);
    std::vector<uint32_t> tab;
    deep_compose_build(F, (uint32_t)g, W, D, w_n, zq, ood, challenges, &tab, S);
    const uint32_t g_m = air_to_m((uint32_t)g, F.p), h_m = air_to_m((uint32_t)cfg->lde_offset, F.p), omega_m = air_to_m(omega, F.p);
    const uint64_t groups = N / DEEP_ROWS, want = (groups + DEEP_BLOCK - 1) / DEEP_BLOCK;
    if (!grid) grid = (uint32_t)(want < 2048 ? want : 2048);
    if (S == 3) emu_window_lanes<3>(tab.data(), W, D, g_m, F, h_m, omega_m, N, grid, lde, stride, seg, seg_stride, out, out_stride);
    else emu_window_lanes<4>(tab.data(), W, D, g_m, F, h_m, omega_m, N, grid, lde, stride, seg, seg_stride, out, out_stride);
    return SMI_OK;
}

// grid: workgroups of the streaming launch (0: as the library sizes it for 256 compute units)
extern "C" int emu_deep_compose(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, uint32_t n_segments, const uint32_t *lde, uint64_t stride, const uint32_t *seg,
                                uint64_t seg_stride, const uint64_t *z, const uint64_t *ood, const uint64_t *challenges, uint32_t *out, uint64_t out_stride,
                                uint32_t grid) {
    FieldSetup fs;
    int rc = SMI_OK;
    if (!setup(p, g, &fs, &rc)) return rc;
    const Fp F = fs.F;
    const uint32_t W = cfg->n_cols, D = n_segments, log_N = cfg->log_n + cfg->log_blowup;
    if (!W || W > 64 || !D || D > DEEP_MAX_SEGMENTS || cfg->log_n < 1 || cfg->log_blowup < 2 || log_N > 27 || log_N > fs.K) return SMI_ERR_BAD_ARG;
    const uint64_t N = 1ull << log_N;
    if (stride < N || seg_stride < N || out_stride < N || !cfg->lde_offset || cfg->lde_offset >= p) return SMI_ERR_BAD_ARG;
    FqH zq;
    if (!point(z, p, &zq)) return SMI_ERR_NON_CANONICAL;
    if (fqh_in_base(zq)) return SMI_ERR_BAD_ARG;
    for (size_t i = 0; i < 4 * (2 * (size_t)W + D); i++)
        if (ood[i] >= p) return SMI_ERR_NON_CANONICAL;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), F.p), omega = host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p);
    std::vector<uint32_t> tab;
    deep_compose_build(F, (uint32_t)g, W, D, w_n, zq, ood, challenges, &tab);
    const uint32_t g_m = air_to_m((uint32_t)g, F.p), h_m = air_to_m((uint32_t)cfg->lde_offset, F.p), omega_m = air_to_m(omega, F.p);
    const uint64_t groups = N / DEEP_ROWS, want = (groups + DEEP_BLOCK - 1) / DEEP_BLOCK;
    if (!grid) grid = (uint32_t)(want < 2048 ? want : 2048);
    const uint64_t gstep = (uint64_t)grid * DEEP_BLOCK;
    const uint32_t xstep_m = mont_pow(omega_m, gstep * DEEP_ROWS, F);
    for (uint64_t gid = 0; gid < gstep && gid < groups; gid++) {
        uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * DEEP_ROWS, F), F);
        for (uint64_t gq = gid; gq < groups; gq += gstep) {
            const uint64_t i0 = gq * DEEP_ROWS;
            uint32_t o[4][DEEP_ROWS];
            deep_compose_points(
                tab.data(), W, D, g_m, F, x_m, omega_m, [&](uint32_t c, uint32_t v[4]) { load4(lde + (uint64_t)c * stride, i0, N, v); },
                [&](uint32_t col, uint32_t v[4]) { load4(seg + (uint64_t)col * seg_stride, i0, N, v); }, o);
            for (int e = 0; e < 4; e++) store4(out + e * out_stride, i0, N, o[e]);
            x_m = mont_mul(x_m, xstep_m, F);
        }
    }
    return SMI_OK;
}

// both sides of the verifier's out-of-domain consistency check (four canonical coordinates each)
extern "C" int emu_deep_ood_sides(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const uint64_t *weights, const uint64_t *z,
                                  const uint64_t *ood, uint64_t *lhs, uint64_t *rhs) {
    FieldSetup fs;
    int rc = SMI_OK;
    if (!setup(p, g, &fs, &rc)) return rc;
    uint32_t D = 0;
    std::string why;
    rc = deep_plan(p, cfg, air, nullptr, &D, &why, SMI_AIR_MAX_WINDOW);
    if (rc != SMI_OK) return rc;
    FqH zq, l, r;
    if (!point(z, p, &zq)) return SMI_ERR_NON_CANONICAL;
    if (fqh_in_base(zq)) return SMI_ERR_BAD_ARG;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), fs.F.p);
    deep_ood_sides((uint32_t)p, (uint32_t)g, cfg, air, D, w_n, weights, zq, ood, &l, &r);
    for (int e = 0; e < 4; e++) lhs[e] = l.c[e], rhs[e] = r.c[e];
    return SMI_OK;
}

// C_k over n_vars = 2 W + 2 Q operands of F_q (four canonical coordinates each, smi_air's numbering)
extern "C" int emu_deep_constraint(uint64_t p, uint64_t g, const smi_air *air, uint32_t k, const uint64_t *operands, uint32_t n_vars, uint64_t *out) {
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30) || k >= air->n_constraints) return SMI_ERR_BAD_ARG;
    for (uint32_t f = 0; f < air->n_factors; f++)
        if (air->factor_var[f] >= n_vars) return SMI_ERR_BAD_ARG;
    std::vector<FqH> X(n_vars);
    for (uint32_t v = 0; v < n_vars; v++)
        if (!point(operands + 4 * (size_t)v, p, &X[v])) return SMI_ERR_NON_CANONICAL;
    const FqH c = deep_constraint(air, k, X.data(), (uint32_t)p, (uint32_t)g);
    for (int e = 0; e < 4; e++) out[e] = c.c[e];
    return SMI_OK;
}

// ... under a window of S rows: ood and gammas hold 4 (S W + D) values
extern "C" int emu_deep_q_at_window(uint64_t p, uint64_t g, uint32_t W, uint32_t D, uint32_t S, uint64_t w_n, uint64_t x, const uint64_t *z, const uint64_t *ood,
                                    const uint64_t *gammas, const uint64_t *trow, const uint64_t *srow, uint64_t *out) {
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30) || S < 2 || S > SMI_AIR_MAX_WINDOW) return SMI_ERR_BAD_ARG;
    FqH zq;
    if (!point(z, p, &zq)) return SMI_ERR_NON_CANONICAL;
    const FqH q = deep_q_at((uint32_t)p, (uint32_t)g, W, D, (uint32_t)w_n, (uint32_t)x, zq, ood, gammas, trow, srow, S);
    for (int e = 0; e < 4; e++) out[e] = q.c[e];
    return SMI_OK;
}

// Q at the point x from the opened rows, as the verifier recomputes it
extern "C" int emu_deep_q_at(uint64_t p, uint64_t g, uint32_t W, uint32_t D, uint64_t w_n, uint64_t x, const uint64_t *z, const uint64_t *ood,
                             const uint64_t *gammas, const uint64_t *trow, const uint64_t *srow, uint64_t *out) {
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30)) return SMI_ERR_BAD_ARG;
    FqH zq;
    if (!point(z, p, &zq)) return SMI_ERR_NON_CANONICAL;
    const FqH q = deep_q_at((uint32_t)p, (uint32_t)g, W, D, (uint32_t)w_n, (uint32_t)x, zq, ood, gammas, trow, srow);
    for (int e = 0; e < 4; e++) out[e] = q.c[e];
    return SMI_OK;
}

// ---- out-of-domain sampling with an argument list (include/stark_mi.h, "Out-of-domain sampling with an argument list")
namespace {
int args_shape(uint64_t p, const FieldSetup &fs, const smi_stark_cfg *cfg, uint32_t A, uint32_t D) {
    const uint32_t W = cfg->n_cols, log_N = cfg->log_n + cfg->log_blowup;
    if (!W || W > 64 || !A || A > SMI_ARGS_MAX || !D || D > DEEP_MAX_SEGMENTS || cfg->log_n < 1 || cfg->log_blowup < 2 || log_N > 27 || log_N > fs.K)
        return SMI_ERR_BAD_ARG;
    if (!cfg->lde_offset || cfg->lde_offset >= p) return SMI_ERR_BAD_ARG;
    return SMI_OK;
}
}  // namespace

// the table of deep_compose_args_kernel as the host builds it: tab gets deep_args_tab_words(W, A, D) words
extern "C" int emu_deep_compose_args_table(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, uint32_t n_args, uint32_t n_segments, const uint64_t *z,
                                           const uint64_t *ood, const uint64_t *challenges, uint32_t *tab_out, uint64_t tab_words) {
    FieldSetup fs;
    int rc = SMI_OK;
    if (!setup(p, g, &fs, &rc)) return rc;
    if ((rc = args_shape(p, fs, cfg, n_args, n_segments)) != SMI_OK) return rc;
    const uint32_t W = cfg->n_cols, A = n_args, D = n_segments;
    if (tab_words != deep_args_tab_words(W, A, D)) return SMI_ERR_BAD_ARG;
    FqH zq;
    if (!point(z, p, &zq)) return SMI_ERR_NON_CANONICAL;
    for (size_t i = 0; i < deep_args_record(W, A, D); i++)
        if (ood[i] >= p) return SMI_ERR_NON_CANONICAL;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), fs.F.p);
    std::vector<uint32_t> tab;
    deep_compose_args_build(fs.F, (uint32_t)g, W, A, D, w_n, zq, ood, challenges, &tab);
    memcpy(tab_out, tab.data(), tab.size() * 4);
    return SMI_OK;
}

// deep_compose_args_kernel's grid-stride loop over deep_compose_args_points.  grid: workgroups of the streaming launch (0: as
// the library sizes it for 256 compute units); with grid = 1 every lane loops once N > DEEP_TILE
extern "C" int emu_deep_compose_args(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, uint32_t n_args, uint32_t n_segments, const uint32_t *lde,
                                     uint64_t stride, const uint32_t *cl, uint64_t c_stride, const uint32_t *seg, uint64_t seg_stride, const uint64_t *z,
                                     const uint64_t *ood, const uint64_t *challenges, uint32_t *out, uint64_t out_stride, uint32_t grid) {
    FieldSetup fs;
    int rc = SMI_OK;
    if (!setup(p, g, &fs, &rc)) return rc;
    if ((rc = args_shape(p, fs, cfg, n_args, n_segments)) != SMI_OK) return rc;
    const Fp F = fs.F;
    const uint32_t W = cfg->n_cols, A = n_args, D = n_segments, log_N = cfg->log_n + cfg->log_blowup;
    const uint64_t N = 1ull << log_N;
    if (stride < N || c_stride < N || seg_stride < N || out_stride < N) return SMI_ERR_BAD_ARG;
    FqH zq;
    if (!point(z, p, &zq)) return SMI_ERR_NON_CANONICAL;
    if (fqh_in_base(zq)) return SMI_ERR_BAD_ARG;
    for (size_t i = 0; i < deep_args_record(W, A, D); i++)
        if (ood[i] >= p) return SMI_ERR_NON_CANONICAL;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), F.p), omega = host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p);
    std::vector<uint32_t> tab;
    deep_compose_args_build(F, (uint32_t)g, W, A, D, w_n, zq, ood, challenges, &tab);
    const uint32_t g_m = air_to_m((uint32_t)g, F.p), h_m = air_to_m((uint32_t)cfg->lde_offset, F.p), omega_m = air_to_m(omega, F.p);
    const uint64_t groups = N / DEEP_ROWS, want = (groups + DEEP_BLOCK - 1) / DEEP_BLOCK;
    if (!grid) grid = (uint32_t)(want < 2048 ? want : 2048);
    const uint64_t gstep = (uint64_t)grid * DEEP_BLOCK;
    const uint32_t xstep_m = mont_pow(omega_m, gstep * DEEP_ROWS, F);
    for (uint64_t gid = 0; gid < gstep && gid < groups; gid++) {
        uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, gid * DEEP_ROWS, F), F);
        for (uint64_t gq = gid; gq < groups; gq += gstep) {
            const uint64_t i0 = gq * DEEP_ROWS;
            uint32_t o[4][DEEP_ROWS];
            deep_compose_args_points(
                tab.data(), W, A, D, g_m, F, x_m, omega_m, [&](uint32_t c, uint32_t v[4]) { load4(lde + (uint64_t)c * stride, i0, N, v); },
                [&](uint32_t col, uint32_t v[4]) { load4(cl + (uint64_t)col * c_stride, i0, N, v); },
                [&](uint32_t col, uint32_t v[4]) { load4(seg + (uint64_t)col * seg_stride, i0, N, v); }, o);
            for (int e = 0; e < 4; e++) store4(out + e * out_stride, i0, N, o[e]);
            x_m = mont_mul(x_m, xstep_m, F);
        }
    }
    return SMI_OK;
}

// Q at the point x from the three opened rows, as the verifier recomputes it
extern "C" int emu_deep_args_q_at(uint64_t p, uint64_t g, uint32_t W, uint32_t A, uint32_t D, uint64_t w_n, uint64_t x, const uint64_t *z, const uint64_t *ood,
                                  const uint64_t *gammas, const uint64_t *trow, const uint64_t *crow, const uint64_t *srow, uint64_t *out) {
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30)) return SMI_ERR_BAD_ARG;
    FqH zq;
    if (!point(z, p, &zq)) return SMI_ERR_NON_CANONICAL;
    const FqH q = deep_args_q_at((uint32_t)p, (uint32_t)g, W, A, D, (uint32_t)w_n, (uint32_t)x, zq, ood, gammas, trow, crow, srow);
    for (int e = 0; e < 4; e++) out[e] = q.c[e];
    return SMI_OK;
}
