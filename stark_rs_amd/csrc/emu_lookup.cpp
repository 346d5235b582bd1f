// emu_lookup.cpp -- CPU emulator of the lookup argument's kernels (TEST INFRASTRUCTURE).
//
// emu_lookup_multiplicities runs the two launches of smi_dev_lookup_multiplicities lane by lane over lookup_insert_lane /
// lookup_count_lane (lookup_core.h) with plain loads and stores where the kernels have atomics; `order` picks the order in
// which the lanes of a launch run (0 ascending, 1 descending, 2 a fixed stride coprime to n), and the result must not
// depend on it.  emu_lookup_column runs the three launches of smi_dev_lookup_column with the kernels' own lane batching and
// block split; emu_air_compose_lookup runs emu_air_compose_ext and then air_lookup_compose_kernel's grid-stride loop over
// lookup_compose_points.  Same arguments and statuses as the C ABI, with (p, g) in place of a context.
#include <string.h>

#include <string>
#include <vector>

#include "lookup_core.h"
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
struct HostAtomics {   // one lane at a time: the atomics are their plain selves
    uint32_t cas(uint32_t *a, uint32_t expect, uint32_t v) const {
        const uint32_t old = *a;
        if (old == expect) *a = v;
        return old;
    }
    void min(uint32_t *a, uint32_t v) const {
        if (v < *a) *a = v;
    }
    void add(uint32_t *a, uint32_t v) const { *a += v; }
};
uint64_t lane_at(uint64_t i, uint64_t n, int order) {
    if (order == 1) return n - 1 - i;
    if (order == 2) return (i * 0x9e3779b1ull + 5) & (n - 1);   // an odd multiplier: a bijection on a power of two
    return i;
}
// lookup_wg_scan of lookup.hip: v[tid] -> excl[tid] and the sum
Fq wg_scan(const Fq *v, Fq *excl, uint32_t p) {
    static thread_local uint32_t sc[2][4][PERM_BLOCK];
    for (uint32_t tid = 0; tid < PERM_BLOCK; tid++)
        for (int e = 0; e < 4; e++) sc[0][e][tid] = v[tid].c[e];
    int cur = 0;
    for (uint32_t off = 1; off < PERM_BLOCK; off <<= 1) {
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) lookup_scan_step(sc[cur], sc[cur ^ 1], tid, off, p);
        cur ^= 1;
    }
    for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) excl[tid] = tid ? perm_scan_at(sc[cur], tid - 1) : Fq{{0, 0, 0, 0}};
    return perm_scan_at(sc[cur], PERM_BLOCK - 1);
}
int lookup_checks(uint64_t p, uint64_t g, const smi_air_lookup *lk, uint32_t n_cols, uint32_t log_n, FieldSetup *fs) {
    if (!field_setup(p, g, fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30)) return SMI_ERR_BAD_ARG;
    if (!n_cols || n_cols > 64 || log_n < 1 || log_n > 27) return SMI_ERR_BAD_ARG;
    return lookup_validate(lk, n_cols, nullptr);
}
}  // namespace

// mult: n words, zeroed here; *missing_row: the smallest row whose lookup tuple is in no table row, or ~0
extern "C" int emu_lookup_multiplicities(uint64_t p, uint64_t g, const smi_air_lookup *lk, const uint32_t *trace, uint32_t n_cols, uint32_t log_n,
                                         uint32_t *mult, int order, uint64_t *missing_row) {
    FieldSetup fs;
    const int rc = lookup_checks(p, g, lk, n_cols, log_n, &fs);
    if (rc != SMI_OK) return rc;
    const uint64_t n = 1ull << log_n, cap = lookup_table_slots(n);
    LookupDev LD;
    const uint64_t no_challenges[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    lookup_build(fs.F, (uint32_t)g, lk, no_challenges, &LD);
    std::vector<uint32_t> tab(cap, LOOKUP_EMPTY);
    memset(mult, 0, n * 4);
    uint64_t first = ~0ull;
    bool exhausted = false;
    for (uint64_t i = 0; i < n; i++)
        if (!lookup_insert_lane(LD, trace, n, tab.data(), (uint32_t)cap, (uint32_t)lane_at(i, n, order), HostAtomics{})) exhausted = true;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t r = lane_at(i, n, order);
        const int got = lookup_count_lane(LD, trace, n, tab.data(), (uint32_t)cap, (uint32_t)r, mult, HostAtomics{});
        if (got == 1 && r < first) first = r;
        if (got == 2) exhausted = true;
    }
    if (missing_row) *missing_row = first;
    if (exhausted) return SMI_ERR_BAD_ARG;
    return first != ~0ull ? SMI_ERR_LOOKUP_MISSING : SMI_OK;
}

// *zero_at: 2 * row + (0: f_L, 1: f_T) of the smallest row with a zero denominator, or ~0
extern "C" int emu_lookup_column(uint64_t p, uint64_t g, const smi_air_lookup *lk, const uint32_t *trace, uint32_t n_cols, uint32_t log_n,
                                 const uint64_t *challenges, uint32_t *s, uint64_t s_stride, int *closes, uint64_t *zero_at) {
    FieldSetup fs;
    const int rc = lookup_checks(p, g, lk, n_cols, log_n, &fs);
    if (rc != SMI_OK) return rc;
    const Fp F = fs.F;
    const uint64_t n = 1ull << log_n, nb = (n + PERM_TILE - 1) / PERM_TILE;
    if (s_stride < n) return SMI_ERR_BAD_ARG;
    LookupDev LD;
    lookup_build(F, (uint32_t)g, lk, challenges, &LD);
    std::vector<Fq> bs(nb);
    uint64_t first = ~0ull;
    // lookup_block_kernel
    std::vector<Fq> sum(PERM_BLOCK), pre(PERM_BLOCK), sls((size_t)PERM_BLOCK * PERM_ROWS);
    for (uint64_t b = 0; b < nb; b++) {
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
            const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
            uint64_t za;
            lookup_lane_column(
                LD, F, row0, n,
                [&](uint32_t col, uint32_t v[4]) {
                    if (row0 < n) load4(trace + (uint64_t)col * n, row0, n, v);
                    else v[0] = v[1] = v[2] = v[3] = 0u;
                },
                &sls[(size_t)tid * PERM_ROWS], &sum[tid], &za);
            if (za < first) first = za;
        }
        bs[b] = wg_scan(sum.data(), pre.data(), F.p);
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
            const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
            if (row0 >= n) break;
            uint32_t o[4][PERM_ROWS];
            for (int q = 0; q < PERM_ROWS; q++) {
                const Fq w = fq_add(sls[(size_t)tid * PERM_ROWS + q], pre[tid], F.p);
                for (int e = 0; e < 4; e++) o[e][q] = w.c[e];
            }
            for (int e = 0; e < 4; e++) store4(s + e * s_stride, row0, n, o[e]);
        }
    }
    // lookup_scan_kernel: one workgroup, PERM_BLOCK sums at a time
    Fq carry{{0, 0, 0, 0}};
    std::vector<Fq> excl(nb);
    for (uint64_t base = 0; base < nb; base += PERM_BLOCK) {
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) sum[tid] = base + tid < nb ? bs[base + tid] : Fq{{0, 0, 0, 0}};
        const Fq tile = wg_scan(sum.data(), pre.data(), F.p);
        for (uint32_t tid = 0; tid < PERM_BLOCK && base + tid < nb; tid++) excl[base + tid] = fq_add(carry, pre[tid], F.p);
        carry = fq_add(carry, tile, F.p);
    }
    // lookup_propagate_kernel
    for (uint64_t b = 0; b < nb; b++)
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
            const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
            if (row0 >= n) break;
            for (int e = 0; e < 4; e++) {
                uint32_t v[PERM_ROWS];
                load4(s + e * s_stride, row0, n, v);
                for (int q = 0; q < PERM_ROWS; q++) v[q] = fp_add(v[q], excl[b].c[e], F.p);
                store4(s + e * s_stride, row0, n, v);
            }
        }
    if (zero_at) *zero_at = first;
    if (first != ~0ull) return SMI_ERR_NO_INVERSE;
    if (closes) *closes = fq_is_zero(carry);
    return SMI_OK;
}

// grid: workgroups of the streaming launch (0: as the library sizes it for 256 compute units)
extern "C" int emu_air_compose_lookup(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_lookup *lk, const uint32_t *lde,
                                      uint64_t stride, const uint32_t *sl, uint64_t s_stride, const uint64_t *challenges, const uint64_t *weights,
                                      uint32_t *out, uint64_t out_stride, int force_direct, uint32_t grid) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr)) return SMI_ERR_BAD_ARG;
    std::string why;
    const int prc = lookup_plan(p, cfg, air, lk, nullptr, nullptr, &why);
    if (prc != SMI_OK) return prc;
    const int rc = emu_air_compose_ext(p, g, cfg, air, lde, stride, weights, out, out_stride, force_direct);
    if (rc != SMI_OK) return rc;
    const uint32_t log_N = cfg->log_n + cfg->log_blowup;
    const Fp F = fs.F;
    AirHost H;
    air_build(F, host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p), cfg, air, &H);
    const AirDev &A = H.dev;
    if (s_stride < A.N) return SMI_ERR_BAD_ARG;
    LookupDev LD;
    lookup_build(F, (uint32_t)g, lk, challenges, &LD);
    const uint64_t *w = weights + 4 * (uint64_t)(A.W + A.K);
    uint32_t wm[4];
    for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[e], F);
    const ExtMul wb = ext_mul_prepare(wm, LD.P.g_m, F);
    for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[4 + e], F);
    const ExtMul wt = ext_mul_prepare(wm, LD.P.g_m, F);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK;
    if (!grid) grid = (uint32_t)(want < 2048 ? want : 2048);
    const uint64_t gstep = (uint64_t)grid * PERM_BLOCK;
    const uint32_t B = 1u << A.log_B, tau_m = air_to_m((uint32_t)cfg->trace_offset, F.p);
    const uint32_t xstep_m = mont_pow(A.omega_m, gstep * PERM_ROWS, F);
    for (uint64_t gid = 0; gid < gstep && gid < groups; gid++) {
        uint32_t x_m = mont_mul(A.h_m, mont_pow(A.omega_m, gid * PERM_ROWS, F), F);
        for (uint64_t gq = gid; gq < groups; gq += gstep) {
            const uint64_t i0 = gq * PERM_ROWS, i1 = (i0 + B) & (A.N - 1);
            uint32_t sc[4][PERM_ROWS], sx[4][PERM_ROWS], acc[4][PERM_ROWS];
            for (int e = 0; e < 4; e++) {
                load4(sl + e * s_stride, i0, A.N, sc[e]);
                load4(sl + e * s_stride, i1, A.N, sx[e]);
                load4(out + e * out_stride, i0, A.N, acc[e]);
            }
            lookup_compose_points(
                LD, F, wb, wt, tau_m, A.izt_m, B, i0, x_m, A.omega_m, [&](uint32_t col, uint32_t v[4]) { load4(lde + (uint64_t)col * stride, i0, A.N, v); }, sc,
                sx, acc);
            for (int e = 0; e < 4; e++) store4(out + e * out_stride, i0, A.N, acc[e]);
            x_m = mont_mul(x_m, xstep_m, F);
        }
    }
    return SMI_OK;
}
